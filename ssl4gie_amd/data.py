"""On-device input pipeline: a uint8 image bank resident in HBM, crop boxes drawn with device-side torch ops, and
one HIP kernel (ops.view_sample_u8) that crops, resamples (PIL's antialiased bicubic / bilinear), flips, clamps and
normalises into the fp32 NCHW batch the models consume.  It stands in for the reference's

    ImageFolder -> RandomResizedCrop(224, scale=(0.2, 1.0), interpolation=3) -> RandomHorizontalFlip -> ToTensor
    -> Normalize  in DataLoader workers, then one host-to-device copy per batch    (Models/mae/main_pretrain.py:123-153)

with no host image work and no image copy: per batch the host sends `batch_size` int64 indices and nothing else.
The geometric part of MoCo-v3's two-view augmentation (Models/moco_v3/main_moco.py:263,275: RandomResizedCrop with
bilinear resampling + flip) is `RandomResizedCropFlip(interpolation="bilinear", scale=(crop_min, 1), mean=(0, 0, 0),
std=(1, 1, 1))`, which yields [0, 1] images; its colour transforms (main_moco.py:264-268,276-281: ColorJitter,
RandomGrayscale, GaussianBlur, Solarize) and the Normalize are `ColorAugment`, a second HIP launch pair
(ops.color_augment) on parameters drawn on the device.  `MoCoV3Views` is the two of them per view, with the two
views' recipes:

    loader = DeviceLoader(bank, 256, sampler=sampler, transform=MoCoV3Views(224, crop_min=0.08))
    for i, (images, _) in enumerate(loader):                            # main_moco.py:311-323, as written
        images[0] = images[0].cuda(gpu, non_blocking=True)              # already there
        images[1] = images[1].cuda(gpu, non_blocking=True)

    bank = DeviceImageBank.from_npy("train_256.npy", "cuda")           # tools/pack_images.py wrote it, once
    sampler = torch.utils.data.DistributedSampler(bank, num_replicas=world, rank=rank, shuffle=True)
    loader = DeviceLoader(bank, 256, sampler=sampler, transform=RandomResizedCropFlip(224))
    for epoch in ...:
        loader.sampler.set_epoch(epoch)
        for it, (samples, _) in enumerate(loader):                      # engine_pretrain.py:39-45, as written
            samples = samples.to(device, non_blocking=True)             # already there: returns itself

The finetune loaders (Binary_segmentation / Depth_estimation / Classification `Data/dataloaders.py`: ColorJitter, a
25-tap GaussianBlur, Normalize, two flips, a nearest-neighbour affine or rotation, the mask or depth map through the
same flips and affine) are `FinetuneAugment`: ops.color_augment_ft, then ops.paired_warp on image and target at once.

    bank = DeviceImageBank.from_npy("train_224.npy", "cuda", targets="train_224_masks.npy")
    loader = DeviceLoader(bank, 16, transform=FinetuneAugment.segmentation())
    for batch_idx, (data, target) in enumerate(loader):                 # Binary_segmentation/train.py, as written
        data, target = data.to(device), target.to(device)               # already there

The detection loaders (Object_detection/Data/dataloaders.py:75-112, Data/dataset.py:38-113 with a fixed size: colour
jitter and the 25-tap blur on the full-resolution image, rot90 and two flips with the boxes carried along, an
antialiased bicubic halving when a side exceeds the fixed size, a centre pad) are `DetectionTransform` over a
`RaggedImageBank` — images of different stored sizes in one flat buffer, with their boxes —: ops.det_color,
ops.det_geometry and ops.det_boxes.  `DetectionLoader` yields the reference's collate_fn tuples:

    bank = RaggedImageBank.from_npy("kvasir_det", "cuda")               # tools/pack_images.py --ragged --boxes wrote it
    loader = DetectionLoader(bank, 4, sampler=sampler, transform=DetectionTransform(1024))
    for images, targets in loader:                                      # train_detection.py:67-69, as written
        images = list(image.cuda(rank) for image in images)             # already there
        targets = [{k: v.cuda(rank) for k, v in t.items()} for t in targets]

The MAE fine-tuning recipe mixes batches that are already on the device (Models/mae/main_finetune.py:221-226,
engine_finetune.py:53): `Mixup` takes timm.data.Mixup's keywords, draws lambda, the mixup / cutmix choice and the boxes
on the host (`mixup_tables`, a pure function of a numpy RandomState), uploads them in one small copy and mixes the
batch in place with one launch of ops.mixup; ops.mixup_target builds the soft targets.

    mixup_fn = Mixup(mixup_alpha=0.8, cutmix_alpha=1.0, label_smoothing=0.1, num_classes=1000)
    samples, targets = mixup_fn(samples, targets)                       # engine_finetune.py:53, as written

The input of that recipe (Models/mae/util/datasets.py:25-66: timm's create_transform with auto_augment=
'rand-m9-mstd0.5-inc1', bicubic, re_prob=0.25, re_mode='pixel', re_count=1) is `MAEFinetuneTransform`: the crop and
flip of `RandomResizedCropFlip` in 0..255 units, ops.quantize_u8 to the bank's uint8 layout, one ops.randaug_layer per
RandAugment layer on op ids, arguments and AFFINE matrices drawn on the device (`RandAugment`), and
ops.normalize_erase_u8, which is ToTensor + Normalize + `RandomErasing` in one pass.  The pixel rules are PIL's, bit
for bit; timm's op list and level maps are restated from its published source.

    bank = DeviceImageBank.from_npy("train_256.npy", "cuda", labels="train_labels.npy")
    loader = DeviceLoader(bank, 256, sampler=sampler_train, transform=MAEFinetuneTransform(224))
    val = DeviceLoader(DeviceImageBank.from_npy("val_256.npy", "cuda", labels="val_labels.npy"), 256,
                       sampler=sampler_val, drop_last=False, transform=MAEFinetuneTransform.eval(224))
    for data_iter_step, (samples, targets) in enumerate(loader):        # engine_finetune.py:42-53, as written
        samples = samples.to(device, non_blocking=True)                 # already there
        targets = targets.to(device, non_blocking=True)
        if mixup_fn is not None:
            samples, targets = mixup_fn(samples, targets)

The MAE linear probe's input (Models/mae/main_linprobe.py:132-141) is `MAELinprobeTransform`: the same crop kernel on
boxes drawn by util/crop.py's one-draw rule (`tf_rrc_boxes`, `RandomResizedCropFlip(sampler="tf")`), flip, Normalize.
MoCo-v3's lincls train input (main_lincls.py:270-277) is `RandomResizedCropFlip(224, scale=(0.08, 1.0),
interpolation="bilinear")` as it stands.
"""
from __future__ import annotations

import functools
import math

import numpy as np
import torch

from . import ops
from .ops import IMAGENET_MEAN, IMAGENET_STD


class DeviceImageBank:
    """[n, Hs, Ws, 3] uint8 images (one stored size) on a device, with optional integer labels and optional
    per-pixel targets [n, Hs, Ws] (masks: uint8, v / 255; depth maps: uint16 — or the same bits in int16 storage —,
    v / 65535; or fp32 as it is).  A map-style dataset whose items are (index, label): torch's own samplers
    (RandomSampler, DistributedSampler and its set_epoch) work on it unchanged, and what they hand out is what
    DeviceLoader sends to the device."""

    TARGET_DTYPES = (torch.uint8, torch.uint16, torch.int16, torch.float32)

    def __init__(self, images_u8, labels=None, targets=None):
        if not (torch.is_tensor(images_u8) and images_u8.dtype == torch.uint8 and images_u8.dim() == 4
                and images_u8.shape[3] == 3 and images_u8.is_contiguous() and images_u8.shape[0] >= 1):
            raise ValueError("DeviceImageBank needs a contiguous uint8 tensor [n, Hs, Ws, 3], n >= 1")
        self.images = images_u8
        n = images_u8.shape[0]
        if labels is None:
            self._labels_host = None
            self.labels = torch.zeros(n, dtype=torch.int64, device=images_u8.device)
        else:
            host = torch.as_tensor(np.asarray(labels.cpu() if torch.is_tensor(labels) else labels)).to(torch.int64)
            if tuple(host.shape) != (n,):
                raise ValueError(f"labels must have shape ({n},), got {tuple(host.shape)}")
            self._labels_host = host.tolist()
            self.labels = host.to(images_u8.device)
        if targets is not None and not (
                torch.is_tensor(targets) and targets.dtype in self.TARGET_DTYPES and targets.is_contiguous()
                and tuple(targets.shape) == tuple(images_u8.shape[:3]) and targets.device == images_u8.device):
            raise ValueError(f"targets must be a contiguous uint8, uint16, int16 or float32 tensor "
                             f"{tuple(images_u8.shape[:3])} on the images' device")
        self.targets = targets

    device = property(lambda self: self.images.device)
    stored_size = property(lambda self: (int(self.images.shape[1]), int(self.images.shape[2])))

    def __len__(self):
        return int(self.images.shape[0])

    def __getitem__(self, i):
        i = int(i)
        if not 0 <= i < len(self):
            raise IndexError(i)
        return i, (0 if self._labels_host is None else self._labels_host[i])

    @classmethod
    def from_uint8(cls, array_or_tensor, device, labels=None, targets=None):
        as_tensor = lambda a: a if torch.is_tensor(a) else torch.from_numpy(np.ascontiguousarray(a))
        t = as_tensor(array_or_tensor)
        if targets is not None:
            targets = as_tensor(targets).contiguous().to(device)
        return cls(t.contiguous().to(device), labels, targets)

    @classmethod
    def from_npy(cls, path, device, labels=None, chunk_bytes=256 << 20, targets=None):
        """`path` is a .npy of [n, Hs, Ws, 3] uint8, `targets` (optional) one of [n, Hs, Ws] uint8, uint16 or float32
        (tools/pack_images.py writes both).  The files are memory-mapped and copied chunk by chunk, so the host never
        holds a second copy of them."""
        def to_device(arr):
            dst = torch.empty(arr.shape, dtype=getattr(torch, arr.dtype.name), device=device)
            step = max(1, int(chunk_bytes) // max(1, int(np.prod(arr.shape[1:])) * arr.dtype.itemsize))
            for a in range(0, arr.shape[0], step):
                dst[a:a + step].copy_(torch.from_numpy(np.array(arr[a:a + step])))
            return dst

        arr = np.load(path, mmap_mode="r")
        if arr.dtype != np.uint8 or arr.ndim != 4 or arr.shape[3] != 3:
            raise ValueError(f"{path}: expected uint8 [n, Hs, Ws, 3], got {arr.dtype} {arr.shape}")
        if targets is not None:
            tgt = np.load(targets, mmap_mode="r")
            if tgt.dtype not in (np.uint8, np.uint16, np.float32) or tgt.shape != arr.shape[:3]:
                raise ValueError(f"{targets}: expected uint8, uint16 or float32 {arr.shape[:3]}, got {tgt.dtype} {tgt.shape}")
            targets = to_device(tgt)
        if isinstance(labels, str):
            labels = np.load(labels)
        return cls(to_device(arr), labels, targets)


class RaggedImageBank:
    """uint8 HWC images of DIFFERENT sizes in one flat device buffer, and their ground-truth boxes: the stored form of
    a detection dataset.  pixels uint8 [total]; image i is the dense rows (3 W bytes each) at offsets[i] (int64 [n], each
    a multiple of 16, derived from the sizes) and is sizes[i] = (H, W) (int32 [n, 2]).  boxes fp32 [m, 4] = (xmin, ymin,
    xmax, ymax) in stored-image pixels, image i owning rows box_offsets[i] .. box_offsets[i + 1] (int64 [n + 1]);
    box_labels int64 [m], all 1 by default (train_detection.py:154-166: one class).  `sizes_host` / `box_offsets_host`
    are host copies (lists), so that grids and the per-image split need no read-back.  A map-style dataset like
    DeviceImageBank: items are (index, 0), torch's samplers and set_epoch work unchanged."""

    ALIGN = 16
    MIN_SIDE = 13   # the 25-tap blur reflects 12 pixels

    @staticmethod
    def offsets_of(sizes):
        """int64 numpy [n] and the total byte count: each image starts at the next multiple of 16"""
        sizes = np.asarray(sizes, dtype=np.int64).reshape(-1, 2)
        nbytes = (sizes[:, 0] * sizes[:, 1] * 3 + RaggedImageBank.ALIGN - 1) // RaggedImageBank.ALIGN * RaggedImageBank.ALIGN
        ends = np.cumsum(nbytes)
        return (ends - nbytes).astype(np.int64), int(ends[-1]) if len(ends) else 0

    def __init__(self, pixels, sizes, boxes, box_offsets, box_labels=None):
        if not (torch.is_tensor(pixels) and pixels.dtype == torch.uint8 and pixels.dim() == 1 and pixels.is_contiguous()):
            raise ValueError("RaggedImageBank needs pixels as a contiguous uint8 vector")
        if not (torch.is_tensor(sizes) and sizes.dtype == torch.int32 and sizes.dim() == 2 and sizes.shape[1] == 2
                and sizes.shape[0] >= 1):
            raise ValueError("sizes must be an int32 tensor [n, 2], n >= 1")
        n = int(sizes.shape[0])
        self.sizes_host = [(int(h), int(w)) for h, w in sizes.cpu().tolist()]
        if min(min(hw) for hw in self.sizes_host) < self.MIN_SIDE:
            raise ValueError(f"every side must be >= {self.MIN_SIDE} (the 25-tap blur reflects 12 pixels)")
        offsets, total = self.offsets_of(self.sizes_host)
        if pixels.numel() != total:
            raise ValueError(f"pixels holds {pixels.numel()} bytes, the sizes need {total} (each image at a multiple of 16)")
        if not (torch.is_tensor(boxes) and boxes.dtype == torch.float32 and boxes.dim() == 2 and boxes.shape[1] == 4):
            raise ValueError("boxes must be a float32 tensor [m, 4]")
        if not (torch.is_tensor(box_offsets) and box_offsets.dtype == torch.int64 and tuple(box_offsets.shape) == (n + 1,)):
            raise ValueError(f"box_offsets must be an int64 tensor [{n + 1}]")
        self.box_offsets_host = [int(v) for v in box_offsets.cpu().tolist()]
        if self.box_offsets_host[0] != 0 or any(b < a for a, b in zip(self.box_offsets_host, self.box_offsets_host[1:])):
            raise ValueError("box_offsets must start at 0 and never decrease")
        m = int(boxes.shape[0])
        if self.box_offsets_host[-1] != m:
            raise ValueError(f"{m} boxes, but box_offsets[-1] = {self.box_offsets_host[-1]}")
        dev = pixels.device
        if box_labels is None:
            box_labels = torch.ones(m, dtype=torch.int64, device=dev)
        elif not (torch.is_tensor(box_labels) and box_labels.dtype == torch.int64 and tuple(box_labels.shape) == (m,)):
            raise ValueError(f"box_labels must be an int64 tensor [{m}]")
        self.pixels, self.sizes = pixels, sizes.contiguous().to(dev)
        self.offsets = torch.from_numpy(offsets).to(dev)
        self.boxes, self.box_offsets = boxes.contiguous().to(dev), box_offsets.contiguous().to(dev)
        self.box_labels = box_labels.contiguous().to(dev)
        self.offsets_host = offsets.tolist()
        self.max_hw = (max(h for h, _ in self.sizes_host), max(w for _, w in self.sizes_host))
        self.max_pixels = max(h * w for h, w in self.sizes_host)

    device = property(lambda self: self.pixels.device)
    targets = None

    def __len__(self):
        return len(self.sizes_host)

    def __getitem__(self, i):
        i = int(i)
        if not 0 <= i < len(self):
            raise IndexError(i)
        return i, 0

    def image(self, i):
        """uint8 [H, W, 3] view of image i"""
        i, _ = self[i]
        (h, w), o = self.sizes_host[i], self.offsets_host[i]
        return self.pixels[o:o + h * w * 3].view(h, w, 3)

    @staticmethod
    def _box_arrays(boxes_per_image, n):
        if len(boxes_per_image) != n:
            raise ValueError(f"{len(boxes_per_image)} box arrays for {n} images")
        arrs = []
        for b in boxes_per_image:
            b = np.asarray(b, dtype=np.float32)
            b = b.reshape(0, 4) if b.size == 0 else b
            if b.ndim != 2 or b.shape[1] != 4:
                raise ValueError(f"boxes of an image must be [k, 4], got {b.shape}")
            arrs.append(b)
        counts = np.array([len(b) for b in arrs], dtype=np.int64)
        return (np.concatenate(arrs, axis=0) if arrs else np.zeros((0, 4), np.float32)), \
            np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)

    @classmethod
    def from_arrays(cls, images, boxes_per_image, device, box_labels=None):
        """images: a list of HWC uint8 arrays; boxes_per_image: a list of [k, 4] arrays, one per image (k may be 0)"""
        if len(images) < 1:
            raise ValueError("RaggedImageBank needs at least one image")
        for a in images:
            if not (isinstance(a, np.ndarray) and a.dtype == np.uint8 and a.ndim == 3 and a.shape[2] == 3
                    and a.flags["C_CONTIGUOUS"]):
                raise ValueError("every image must be a C-contiguous uint8 array [H, W, 3]")
        sizes = np.array([a.shape[:2] for a in images], dtype=np.int32)
        offsets, total = cls.offsets_of(sizes)
        flat = np.zeros(total, dtype=np.uint8)
        for a, o in zip(images, offsets):
            flat[o:o + a.size] = a.reshape(-1)
        boxes, box_offsets = cls._box_arrays(boxes_per_image, len(images))
        labels = None if box_labels is None else torch.as_tensor(np.asarray(box_labels), dtype=torch.int64)
        return cls(torch.from_numpy(flat).to(device), torch.from_numpy(sizes), torch.from_numpy(boxes),
                   torch.from_numpy(box_offsets), labels)

    @classmethod
    def from_npy(cls, prefix, device, chunk_bytes=256 << 20):
        """<prefix>.pixels.npy, .sizes.npy, .boxes.npy, .box_offsets.npy as tools/pack_images.py --ragged writes them.
        The pixel file is memory-mapped and copied chunk by chunk, so the host never holds a second copy of it."""
        arr = np.load(prefix + ".pixels.npy", mmap_mode="r")
        if arr.dtype != np.uint8 or arr.ndim != 1:
            raise ValueError(f"{prefix}.pixels.npy: expected a uint8 vector, got {arr.dtype} {arr.shape}")
        sizes, boxes = np.load(prefix + ".sizes.npy"), np.load(prefix + ".boxes.npy")
        box_offsets = np.load(prefix + ".box_offsets.npy")
        if sizes.dtype != np.int32 or boxes.dtype != np.float32 or box_offsets.dtype != np.int64:
            raise ValueError(f"{prefix}: expected int32 sizes, float32 boxes and int64 box_offsets, got {sizes.dtype}, "
                             f"{boxes.dtype}, {box_offsets.dtype}")
        dst = torch.empty(arr.shape[0], dtype=torch.uint8, device=device)
        step = max(1, int(chunk_bytes))
        for a in range(0, arr.shape[0], step):
            dst[a:a + step].copy_(torch.from_numpy(np.array(arr[a:a + step])))
        return cls(dst, torch.from_numpy(sizes), torch.from_numpy(boxes), torch.from_numpy(box_offsets))


@functools.lru_cache(maxsize=64)
def _fallback_box(Hs, Ws, ratio, device):
    """get_params' box when none of the 10 tries fits: centred, of the nearest allowed aspect.  A constant of
    (stored size, ratio): built once per device, so that no draw carries a host-to-device copy."""
    in_ratio = Ws / Hs
    if in_ratio < min(ratio):
        fw, fh = Ws, int(round(Ws / min(ratio)))
    elif in_ratio > max(ratio):
        fh, fw = Hs, int(round(Hs * max(ratio)))
    else:
        fw, fh = Ws, Hs
    return torch.tensor([(Hs - fh) // 2, (Ws - fw) // 2, fh, fw], dtype=torch.float64, device=device)


def rrc_boxes(u, Hs, Ws, scale=(0.2, 1.0), ratio=(3.0 / 4.0, 4.0 / 3.0)):
    """transforms.RandomResizedCrop.get_params as a pure function of uniforms u [B, 10, 4] in [0, 1): per try
    (area fraction, log-aspect, top, left).  float64 on u's device, vectorised, no host read-back.  Returns int32
    [B, 4] = (top, left, height, width).  torchvision draws its scalars one at a time, so its random SEQUENCE
    is not reproduced; its distribution is."""
    assert u.dim() == 3 and tuple(u.shape[1:]) == (10, 4)
    u = u.to(torch.float64)
    area = float(Hs * Ws)
    l0, l1 = math.log(ratio[0]), math.log(ratio[1])
    target = area * (scale[0] + u[..., 0] * (scale[1] - scale[0]))
    aspect = torch.exp(l0 + u[..., 1] * (l1 - l0))
    w = torch.round(torch.sqrt(target * aspect))          # round half to even, as Python's round()
    h = torch.round(torch.sqrt(target / aspect))
    ok = (w > 0) & (w <= Ws) & (h > 0) & (h <= Hs)
    top = torch.minimum(torch.floor(u[..., 2] * (Hs - h + 1)), Hs - h)   # (u < 1: the minimum never binds)
    left = torch.minimum(torch.floor(u[..., 3] * (Ws - w + 1)), Ws - w)
    first = torch.argmax(ok.to(torch.uint8), dim=1)       # the first try that fits (argmax returns the first maximum)
    tries = torch.stack([top, left, h, w], dim=2)         # [B, 10, 4]
    won = tries.gather(1, first.view(-1, 1, 1).expand(-1, 1, 4)).squeeze(1)
    fallback = _fallback_box(int(Hs), int(Ws), (float(ratio[0]), float(ratio[1])), u.device)
    return torch.where(ok.any(dim=1, keepdim=True), won, fallback).to(torch.int32)


@functools.lru_cache(maxsize=64)
def _log_ratio_f32(ratio):
    """torch.log(torch.tensor(ratio)) of util/crop.py:28 — fp32 — as two Python floats (a host constant of `ratio`)"""
    lr = torch.log(torch.tensor(ratio, dtype=torch.float32))
    return float(lr[0]), float(lr[1])


def tf_rrc_boxes(u, Hs, Ws, scale=(0.08, 1.0), ratio=(3.0 / 4.0, 4.0 / 3.0)):
    """The MAE linear probe's RandomResizedCrop.get_params (reference Models/mae/util/crop.py:23-42, "for matching
    TF/TPU implementation: no for-loop is used"): ONE draw, clamped to the image, where torchvision's rule (rrc_boxes)
    retries up to ten times and falls back to a centred box.  A pure function of uniforms u [B, 4] in [0, 1): area
    fraction, log-aspect, top, left.  The log-ratio bounds and the exp are fp32, as the reference's are; everything
    else is float64 on u's device, vectorised, no host read-back.  round() is half-to-even, as Python's.  Returns int32
    [B, 4] = (top, left, height, width).  The reference draws its scalars one at a time from torch's global generator,
    so its random SEQUENCE is not reproduced; its distribution is.  (A side that rounds to 0 — an image of a few
    pixels, where the reference's crop fails — is raised to 1.)"""
    assert u.dim() == 2 and u.shape[1] == 4
    u = u.to(torch.float64)
    l0, l1 = _log_ratio_f32((float(ratio[0]), float(ratio[1])))
    target = float(Hs * Ws) * (scale[0] + u[:, 0] * (scale[1] - scale[0]))
    aspect = torch.exp((l0 + u[:, 1] * (l1 - l0)).to(torch.float32)).to(torch.float64)
    w = torch.round(torch.sqrt(target * aspect)).clamp(1, Ws)
    h = torch.round(torch.sqrt(target / aspect)).clamp(1, Hs)
    top = torch.minimum(torch.floor(u[:, 2] * (Hs - h + 1)), Hs - h)     # torch.randint(0, height - h + 1)
    left = torch.minimum(torch.floor(u[:, 3] * (Ws - w + 1)), Ws - w)
    return torch.stack([top, left, h, w], dim=1).to(torch.int32)


class RandomResizedCropFlip:
    """RandomResizedCrop(size, scale, ratio, interpolation) + RandomHorizontalFlip(flip_p) + ToTensor +
    Normalize(mean, std), drawn and computed on the bank's device.  __call__(bank, index) -> [B, 3, size, size]
    fp32, or a list of `views` independently drawn such batches when views > 1.  sampler: the box rule —
    "torchvision" (rrc_boxes: ten tries and a fallback) or "tf" (tf_rrc_boxes: the MAE linear probe's one draw)."""

    def __init__(self, size=224, scale=(0.2, 1.0), ratio=(3.0 / 4.0, 4.0 / 3.0), interpolation="bicubic", flip_p=0.5,
                 views=1, mean=IMAGENET_MEAN, std=IMAGENET_STD, generator=None, sampler="torchvision"):
        if interpolation not in ("bicubic", "bilinear"):
            raise ValueError(f"interpolation must be 'bicubic' or 'bilinear', got {interpolation!r}")
        if sampler not in ("torchvision", "tf"):
            raise ValueError(f"sampler must be 'torchvision' or 'tf', got {sampler!r}")
        if size % 4 or views < 1:
            raise ValueError("size must be a multiple of 4 and views >= 1")
        self.size, self.scale, self.ratio, self.interpolation = int(size), tuple(scale), tuple(ratio), interpolation
        self.flip_p, self.views, self.mean, self.std, self.generator = float(flip_p), int(views), tuple(mean), tuple(std), generator
        self.sampler = sampler

    def draw(self, B, Hs, Ws, device):
        """one view's boxes int32 [B, 4] and flips uint8 [B] (advances the generator)"""
        if self.sampler == "tf":
            u = torch.rand(B, 4, dtype=torch.float64, device=device, generator=self.generator)
            v = torch.rand(B, dtype=torch.float64, device=device, generator=self.generator)
            return tf_rrc_boxes(u, Hs, Ws, self.scale, self.ratio), (v < self.flip_p).to(torch.uint8)
        u = torch.rand(B, 10, 4, dtype=torch.float64, device=device, generator=self.generator)
        v = torch.rand(B, dtype=torch.float64, device=device, generator=self.generator)
        return rrc_boxes(u, Hs, Ws, self.scale, self.ratio), (v < self.flip_p).to(torch.uint8)

    def _view(self, bank, index):
        Hs, Ws = bank.stored_size
        box, flip = self.draw(index.shape[0], Hs, Ws, index.device)
        return ops.view_sample_u8(bank.images, index, box, flip, self.size, self.interpolation, self.mean, self.std)

    def __call__(self, bank, index):
        if self.views == 1:
            return self._view(bank, index)
        return [self._view(bank, index) for _ in range(self.views)]


class ColorAugment:
    """RandomApply([ColorJitter(brightness, contrast, saturation, hue)], jitter_p) + RandomGrayscale(gray_p) +
    RandomApply([GaussianBlur(blur_sigma)], blur_p) + RandomApply([Solarize()], solarize_p) + Normalize(mean, std)
    (Models/moco_v3/main_moco.py:264-271) on a device batch x fp32 [B, 3, S, S] in [0, 1], one parameter set per
    sample drawn on x's device.  The defaults are MoCo-v3's first view.  The blur is a true Gaussian of radius
    ceil(3 sigma) <= 6 pixels, hence blur_sigma[1] <= 2 (the reference's range)."""

    def __init__(self, brightness=0.4, contrast=0.4, saturation=0.2, hue=0.1, jitter_p=0.8, gray_p=0.2, blur_p=1.0,
                 blur_sigma=(0.1, 2.0), solarize_p=0.0, mean=IMAGENET_MEAN, std=IMAGENET_STD, generator=None):
        if min(brightness, contrast, saturation, hue) < 0:
            raise ValueError("brightness, contrast, saturation and hue must be >= 0")
        if hue > 0.5:
            raise ValueError(f"hue must be <= 0.5, got {hue}")
        if not 0 <= blur_sigma[0] <= blur_sigma[1]:
            raise ValueError(f"blur_sigma must be 0 <= lo <= hi, got {tuple(blur_sigma)}")
        if blur_sigma[1] > 2.0:
            raise ValueError(f"blur_sigma[1] must be <= 2.0 (a radius of 6 pixels), got {blur_sigma[1]}")
        if not all(0.0 <= p <= 1.0 for p in (jitter_p, gray_p, blur_p, solarize_p)):
            raise ValueError("probabilities must lie in [0, 1]")
        self.jitter = (float(brightness), float(contrast), float(saturation), float(hue))
        self.jitter_p, self.gray_p, self.blur_p, self.solarize_p = float(jitter_p), float(gray_p), float(blur_p), float(solarize_p)
        self.blur_sigma = (float(blur_sigma[0]), float(blur_sigma[1]))
        self.mean, self.std, self.generator = tuple(mean), tuple(std), generator

    def ranges(self):
        """[(lo, hi)] of the brightness, contrast, saturation and hue factors (ColorJitter._check_input)"""
        b, c, s, h = self.jitter
        return [(max(0.0, 1.0 - v), 1.0 + v) for v in (b, c, s)] + [(-h, h)]

    def draw(self, B, device):
        """factors fp32 [B, 4], order uint8 [B, 4], flags uint8 [B], sigma fp32 [B] (advances the generator).
        ColorJitter.get_params: a uniform random permutation of the four ops (argsort of uniforms) and one uniform
        factor each; an op whose range is a point (value 0) is left out, as torchvision leaves it out.  Vectorised
        on the device, no host read-back; torchvision's random SEQUENCE is not reproduced, its distribution is."""
        u = torch.rand(B, 13, dtype=torch.float64, device=device, generator=self.generator)
        on = (u[:, 8] < self.jitter_p).unsqueeze(1)
        order = torch.argsort(u[:, 0:4], dim=1).to(torch.uint8)
        cols = []
        for k, (lo, hi) in enumerate(self.ranges()):
            cols.append(lo + u[:, 4 + k] * (hi - lo))
            if self.jitter[k] == 0.0:
                order = order.masked_fill(order == k, 255)
        factors = torch.stack([torch.where(on[:, 0], c, 1.0 if k < 3 else 0.0) for k, c in enumerate(cols)], dim=1)
        order = order.masked_fill(~on, 255)
        flags = (u[:, 9] < self.gray_p).to(torch.uint8) + 2 * (u[:, 11] < self.solarize_p).to(torch.uint8)
        lo, hi = self.blur_sigma
        sigma = torch.where(u[:, 10] < self.blur_p, lo + u[:, 12] * (hi - lo), 0.0)
        return factors.to(torch.float32).contiguous(), order.contiguous(), flags, sigma.to(torch.float32)

    def __call__(self, x):
        return ops.color_augment(x, *self.draw(x.shape[0], x.device), self.mean, self.std)


class MoCoV3Views:
    """MoCo-v3's two-view transform (Models/moco_v3/main_moco.py:262-285) for DeviceLoader: per view a
    RandomResizedCropFlip(size, scale=(crop_min, 1), bilinear) into [0, 1] and that view's ColorAugment — view 1
    always blurred, view 2 blurred with p = 0.1 and solarized with p = 0.2.  __call__(bank, index) -> [view1, view2],
    as the MoCo loop indexes them.  The one generator is drawn from in the order crop 1, colour 1, crop 2, colour 2."""

    def __init__(self, size=224, crop_min=0.08, mean=IMAGENET_MEAN, std=IMAGENET_STD, generator=None):
        self.crops = [RandomResizedCropFlip(size, scale=(crop_min, 1.0), interpolation="bilinear", mean=(0.0, 0.0, 0.0),
                                            std=(1.0, 1.0, 1.0), generator=generator) for _ in range(2)]
        self.colors = [ColorAugment(blur_p=1.0, solarize_p=0.0, mean=mean, std=std, generator=generator),
                       ColorAugment(blur_p=0.1, solarize_p=0.2, mean=mean, std=std, generator=generator)]

    def __call__(self, bank, index):
        return [color(crop(bank, index)) for crop, color in zip(self.crops, self.colors)]


def affine_matrices(angle, translate=None, scale=None, shear=None, dtype=torch.float32):
    """torchvision's _get_inverse_affine_matrix(center=(0, 0), angle, translate, scale, shear=(shear, 0)) — the matrix
    TF.affine hands its tensor path — for a batch: angle [B] and shear [B] in degrees, translate [B, 2] = (tx, ty) in
    pixels, scale [B]; None = 0, (0, 0), 1, 0.  float64 on angle's device, vectorised, no host read-back.  Returns
    [B, 6] in `dtype` (fp32 is what the kernel takes): the map from centred OUTPUT coordinates to centred source coordinates that ops.paired_warp takes.
    TF.rotate(angle) is affine_matrices(-angle)."""
    rot = torch.deg2rad(angle.to(torch.float64))
    sx = torch.zeros_like(rot) if shear is None else torch.deg2rad(shear.to(torch.float64))
    sc = torch.ones_like(rot) if scale is None else scale.to(torch.float64)
    t = torch.zeros(rot.shape[0], 2, dtype=torch.float64, device=rot.device) if translate is None else translate.to(torch.float64)
    # with sy = 0: a = cos(rot), c = sin(rot)
    a, c = torch.cos(rot), torch.sin(rot)
    b = -torch.cos(rot) * torch.tan(sx) - torch.sin(rot)
    d = -torch.sin(rot) * torch.tan(sx) + torch.cos(rot)
    m0, m1, m3, m4 = d / sc, -b / sc, -c / sc, a / sc
    m2 = m0 * -t[:, 0] + m1 * -t[:, 1]
    m5 = m3 * -t[:, 0] + m4 * -t[:, 1]
    return torch.stack([m0, m1, m2, m3, m4, m5], dim=1).to(dtype).contiguous()


class FinetuneAugment:
    """The train-time augmentation of the reference's finetune loaders for DeviceLoader, drawn and computed on the
    bank's device: ColorJitter(brightness, contrast, saturation, hue) (always applied) -> GaussianBlur((25, 25),
    blur_sigma) (None: no blur) -> ToTensor -> Normalize(mean, std) -> horizontal and vertical flip, each when a
    uniform draw exceeds 0.5 -> TF.affine(angle U(-a, a), translate U(-t size, t size)^2, scale U(lo, hi), shear
    U(-s, s)), nearest, the image filled with `fill` (a number in normalised space, or "black" = the normalised value
    of a black pixel) and the target with 0.  `affine` is None or a dict with any of angle, translate (a fraction of
    the size), scale (lo, hi), shear; keys left out are not drawn (a dict with angle alone is RandomRotation: its range
    is symmetric, so TF.rotate's opposite sign convention draws the same distribution).
    __call__(bank, index) -> images fp32 [B, 3, size, size], or (images, targets fp32 [B, 1, size, size]) for a bank
    with targets, which go through the same flips and affine.  The bank's stored size must be `size`: the reference
    resizes to 224 when it loads a file, tools/pack_images.py does that once."""

    def __init__(self, size=224, brightness=0.4, contrast=0.5, saturation=0.25, hue=0.01, blur_sigma=(0.001, 2.0),
                 hflip=True, vflip=True, affine=None, fill=-1.0, mean=IMAGENET_MEAN, std=IMAGENET_STD, generator=None):
        if size < 16 or size % 4:
            raise ValueError(f"size must be >= 16 and a multiple of 4, got {size}")
        if blur_sigma is not None and not 0 < blur_sigma[0] <= blur_sigma[1]:
            raise ValueError(f"blur_sigma must be None or 0 < lo <= hi, got {tuple(blur_sigma)}")
        affine = None if affine is None else dict(affine)
        if affine is not None and set(affine) - {"angle", "translate", "scale", "shear"}:
            raise ValueError(f"affine takes angle, translate, scale and shear, got {sorted(affine)}")
        if fill != "black" and isinstance(fill, str):
            raise ValueError(f"fill must be a number or 'black', got {fill!r}")
        self.size, self.hflip, self.vflip, self.affine = int(size), bool(hflip), bool(vflip), affine
        self.blur_sigma = None if blur_sigma is None else (float(blur_sigma[0]), float(blur_sigma[1]))
        self.mean, self.std, self.generator = tuple(mean), tuple(std), generator
        self.fill = tuple((0.0 - m) / s for m, s in zip(self.mean, self.std)) if fill == "black" else (float(fill),) * 3
        # the jitter parameters are ColorAugment's draw with nothing else switched on
        self.color = ColorAugment(brightness, contrast, saturation, hue, jitter_p=1.0, gray_p=0.0, blur_p=0.0,
                                  solarize_p=0.0, mean=mean, std=std, generator=generator)

    @classmethod
    def segmentation(cls, size=224, **kw):
        """Binary_segmentation/Data/dataloaders.py:62-87, dataset.py:46-63"""
        kw.setdefault("affine", dict(angle=180.0, translate=1.0 / 8.0, scale=(0.5, 1.5), shear=22.5))
        return cls(size, **kw)

    @classmethod
    def depth(cls, size=224, **kw):
        """Depth_estimation/Data/dataloaders.py:55-65, dataset.py:47-70: jitter and the two flips"""
        kw.setdefault("blur_sigma", None)
        return cls(size, **kw)

    @classmethod
    def classification(cls, size=224, **kw):
        """Classification/Data/dataloaders.py:62-72: jitter, blur, flips, RandomRotation(180) with black fill"""
        kw.setdefault("affine", dict(angle=180.0))
        kw.setdefault("fill", "black")
        return cls(size, **kw)

    def draw(self, B, device):
        """(factors fp32 [B, 4], order uint8 [B, 4], flags uint8 [B], sigma fp32 [B], flip uint8 [B], matrix fp32
        [B, 6]); advances the generator.  No blur: sigma = 0; no affine: identity matrices."""
        factors, order, flags, _ = self.color.draw(B, device)
        u = torch.rand(B, 8, dtype=torch.float64, device=device, generator=self.generator)
        if self.blur_sigma is None:
            sigma = torch.zeros(B, dtype=torch.float32, device=device)
        else:
            lo, hi = self.blur_sigma
            sigma = (lo + u[:, 0] * (hi - lo)).to(torch.float32)
        flip = ((u[:, 1] > 0.5) & self.hflip).to(torch.uint8) + 2 * ((u[:, 2] > 0.5) & self.vflip).to(torch.uint8)
        spread = lambda col, half: (2.0 * u[:, col] - 1.0) * half
        a = self.affine or {}
        angle = spread(3, float(a.get("angle", 0.0)))
        t = float(a.get("translate", 0.0)) * self.size
        lo, hi = a.get("scale", (1.0, 1.0))
        matrix = affine_matrices(angle, torch.stack([spread(4, t), spread(5, t)], dim=1), lo + u[:, 6] * (hi - lo),
                                 spread(7, float(a.get("shear", 0.0))))
        return factors, order, flags, sigma, flip, matrix

    def __call__(self, bank, index):
        if bank.stored_size != (self.size, self.size):
            raise ValueError(f"FinetuneAugment({self.size}) needs a bank stored at {self.size} x {self.size}, got "
                             f"{bank.stored_size}: pack it at that size (tools/pack_images.py --size)")
        factors, order, flags, sigma, flip, matrix = self.draw(index.shape[0], index.device)
        # [0, 1] images: ToTensor.  (view_sample_u8 with the whole image as its box gives these very bits and would
        # save the gathered copy; both multiply by fp32 1 / 255, which is not v / 255 for 126 of the 256 levels.)
        x = ops.normalize_u8(bank.images[index], (0.0, 0.0, 0.0), (1.0, 1.0, 1.0))
        x = ops.color_augment_ft(x, factors, order, flags, sigma, self.mean, self.std)
        if bank.targets is None:
            return ops.paired_warp(x, matrix, flip, self.fill)
        return ops.paired_warp(x, matrix, flip, self.fill, bank.targets, index, 0.0)


class DetectionTransform:
    """The detection train loader (Object_detection/Data/dataloaders.py:75-99, Data/dataset.py:38-113 with arch !=
    "resnet50") for DetectionLoader, drawn and computed on the bank's device: ColorJitter(brightness, contrast,
    saturation, hue) -> GaussianBlur((25, 25), blur_sigma) on the stored image -> ToTensor -> rot90, hflip, vflip, each
    where a uniform draw exceeds 0.5, the boxes carried along -> an antialiased bicubic halving when a side exceeds
    fixed_size -> a centre pad to fixed_size^2 -> (x - mean) / std, the padding being the normalised value of black
    (the reference normalises in the model: mean 0, std 1 here).  DetectionTransform.eval(fixed_size) is the val /
    test loader: ToTensor, the halving and the pad.
    __call__(bank, index) -> (images fp32 [B, 3, F, F], boxes fp32 [sum k, 4], labels int64 [sum k]); the per-sample
    counts are the bank's host copy, index being known on the host too (`index_host`, else it is read back).
    Out of scope: arch = "resnet50" (no fixed size), post_process=True, and a bank with a side above 2 fixed_size
    (the reference's negative pad, a crop)."""

    def __init__(self, fixed_size=1024, brightness=0.4, contrast=0.5, saturation=0.25, hue=0.01,
                 blur_sigma=(0.001, 2.0), rotate=True, hflip=True, vflip=True, mean=(0.0, 0.0, 0.0),
                 std=(1.0, 1.0, 1.0), generator=None, color=True):
        if fixed_size < 4 or fixed_size % 4:
            raise ValueError(f"fixed_size must be a multiple of 4, got {fixed_size}")
        if blur_sigma is not None and not 0 < blur_sigma[0] <= blur_sigma[1]:
            raise ValueError(f"blur_sigma must be None or 0 < lo <= hi, got {tuple(blur_sigma)}")
        if len(mean) != 3 or len(std) != 3 or any(float(v) == 0.0 for v in std):
            raise ValueError("mean and std must hold three values, std none equal to 0")
        self.fixed_size, self.rotate, self.hflip, self.vflip = int(fixed_size), bool(rotate), bool(hflip), bool(vflip)
        self.blur_sigma = None if blur_sigma is None else (float(blur_sigma[0]), float(blur_sigma[1]))
        self.mean, self.std, self.generator = tuple(float(v) for v in mean), tuple(float(v) for v in std), generator
        # the jitter parameters are ColorAugment's draw with nothing else switched on, as in FinetuneAugment
        self.color = None if not color else ColorAugment(brightness, contrast, saturation, hue, jitter_p=1.0, gray_p=0.0,
                                                         blur_p=0.0, solarize_p=0.0, generator=generator)
        self._scratch = None
        self.last_draw = None

    @classmethod
    def eval(cls, fixed_size=1024, mean=(0.0, 0.0, 0.0), std=(1.0, 1.0, 1.0)):
        """dataloaders.py:116-120: no colour stage, no rotation, no flips"""
        return cls(fixed_size, rotate=False, hflip=False, vflip=False, mean=mean, std=std, color=False)

    def draw(self, B, device):
        """(factors fp32 [B, 4], order uint8 [B, 4], sigma fp32 [B], geom uint8 [B]: bit 0 hflip, bit 1 vflip, bit 2
        rot90); advances the generator.  Without a colour stage the first three are None."""
        factors = order = sigma = None
        if self.color is not None:
            factors, order, _, _ = self.color.draw(B, device)
        u = torch.rand(B, 4, dtype=torch.float64, device=device, generator=self.generator)
        if self.color is not None:
            if self.blur_sigma is None:
                sigma = torch.zeros(B, dtype=torch.float32, device=device)
            else:
                lo, hi = self.blur_sigma
                sigma = (lo + u[:, 0] * (hi - lo)).to(torch.float32)
        geom = (((u[:, 2] > 0.5) & self.hflip).to(torch.uint8) + 2 * ((u[:, 3] > 0.5) & self.vflip).to(torch.uint8)
                + 4 * ((u[:, 1] > 0.5) & self.rotate).to(torch.uint8))
        return factors, order, sigma, geom

    def check(self, bank):
        if not isinstance(bank, RaggedImageBank):
            raise TypeError("DetectionTransform needs a RaggedImageBank")
        if max(bank.max_hw) > 2 * self.fixed_size:
            raise ValueError(f"the bank holds a side of {max(bank.max_hw)} > 2 x fixed_size = {2 * self.fixed_size}: the "
                             "reference's negative pad (a crop) is not supported")

    def __call__(self, bank, index, index_host=None):
        self.check(bank)
        if index_host is None:
            index_host = index.tolist()
        B, F, dev = len(index_host), self.fixed_size, bank.device
        for i in index_host:
            if not 0 <= i < len(bank):
                raise IndexError(i)
        off = bank.box_offsets_host
        counts = [off[i + 1] - off[i] for i in index_host]
        starts = [0]
        for c in counts:
            starts.append(starts[-1] + c)
        self.last_counts = counts
        out_start = torch.tensor(starts, dtype=torch.int64)
        if dev.type != "cpu":
            out_start = out_start.pin_memory()
        out_start = out_start.to(dev, non_blocking=True)
        factors, order, sigma, geom = self.last_draw = self.draw(B, dev)
        scratch = None
        if self.color is not None and B:
            need = (bank.max_pixels + 3) & ~3
            if self._scratch is None or self._scratch.shape[0] < B or self._scratch.shape[2] != need \
                    or self._scratch.device != dev:
                self._scratch = torch.empty(B, 3, need, dtype=torch.float32, device=dev)
            scratch = self._scratch[:B]
            max_hw = (max(bank.sizes_host[i][0] for i in index_host), max(bank.sizes_host[i][1] for i in index_host))
            ops.det_color(bank.pixels, bank.offsets, bank.sizes, index, factors, order, sigma, max_hw, scratch)
        images = ops.det_geometry(bank.pixels, bank.offsets, bank.sizes, index, geom, F, self.mean, self.std, scratch)
        boxes, labels = ops.det_boxes(bank.boxes, bank.box_labels, bank.box_offsets, bank.sizes, index, geom, out_start,
                                      starts[-1], max(counts, default=0), F)
        return images, boxes, labels


class DetectionLoader:
    """The reference's detection DataLoader with its collate_fn (Object_detection/Data/dataloaders.py:12-13, 105-112)
    over a RaggedImageBank: iteration yields (tuple of B images [3, F, F], tuple of B {"boxes": [k, 4], "labels": [k]}
    dicts), every entry a view of the batch's tensors, so train_detection.py:67-69 runs as written and its .cuda(rank)
    calls return the tensors themselves.  The stacked batch of the last iteration is `last_images` ([B, 3, F, F]),
    `last_boxes`, `last_labels`, for callers that feed the backbone directly.  Per batch the host sends the indices
    and the boxes' split points; nothing synchronises."""

    def __init__(self, bank, batch_size, sampler=None, drop_last=True, transform=None):
        if batch_size < 1:
            raise ValueError("batch_size must be >= 1")
        self.bank, self.batch_size, self.drop_last = bank, int(batch_size), bool(drop_last)
        self.sampler = sampler if sampler is not None else torch.utils.data.RandomSampler(bank)
        self.transform = transform if transform is not None else DetectionTransform()
        self.transform.check(bank)
        self.last_images = self.last_boxes = self.last_labels = None

    def __len__(self):
        n = len(self.sampler)
        return n // self.batch_size if self.drop_last else (n + self.batch_size - 1) // self.batch_size

    def _batch(self, idx):
        host = torch.tensor(idx, dtype=torch.int64)
        dev = self.bank.device
        if dev.type != "cpu":
            host = host.pin_memory()
        images, boxes, labels = self.transform(self.bank, host.to(dev, non_blocking=True), idx)
        self.last_images, self.last_boxes, self.last_labels = images, boxes, labels
        counts = self.transform.last_counts
        targets = tuple({"boxes": b, "labels": l} for b, l in zip(boxes.split(counts), labels.split(counts)))
        return tuple(images.unbind(0)), targets

    def __iter__(self):
        idx = []
        for i in self.sampler:
            idx.append(int(i))
            if len(idx) == self.batch_size:
                yield self._batch(idx)
                idx = []
        if idx and not self.drop_last:
            yield self._batch(idx)


class DeviceLoader:
    """What the reference's DataLoader is to its training loops, over a DeviceImageBank: len(), iteration that
    yields (samples, labels) — ([view1, view2], labels) for a two-view transform; (samples, targets) for a bank
    with per-pixel targets, whose transform must return that pair (FinetuneAugment) — and `.sampler` for
    set_epoch.  Per batch the host takes `batch_size` plain ints from the sampler and sends them as one int64
    tensor (pinned, non_blocking); the transform does the rest on the device.  Nothing synchronises."""

    def __init__(self, bank, batch_size, sampler=None, drop_last=True, transform=None):
        if batch_size < 1:
            raise ValueError("batch_size must be >= 1")
        self.bank, self.batch_size, self.drop_last = bank, int(batch_size), bool(drop_last)
        self.sampler = sampler if sampler is not None else torch.utils.data.RandomSampler(bank)
        self.transform = transform if transform is not None else RandomResizedCropFlip()

    def __len__(self):
        n = len(self.sampler)
        return n // self.batch_size if self.drop_last else (n + self.batch_size - 1) // self.batch_size

    def _batch(self, idx):
        host = torch.tensor(idx, dtype=torch.int64)
        dev = self.bank.device
        if dev.type != "cpu":
            host = host.pin_memory()
        index = host.to(dev, non_blocking=True)
        out = self.transform(self.bank, index)
        if self.bank.targets is None:
            return out, self.bank.labels[index]
        if not (isinstance(out, tuple) and len(out) == 2):
            raise TypeError("a bank with targets needs a transform that returns (images, targets), such as FinetuneAugment")
        return out

    def __iter__(self):
        idx = []
        for i in self.sampler:
            idx.append(int(i))
            if len(idx) == self.batch_size:
                yield self._batch(idx)
                idx = []
        if idx and not self.drop_last:
            yield self._batch(idx)


# ------------------------------------------------------------------------------------------------
# The train and eval transforms of the MAE fine-tuning recipe (Models/mae/util/datasets.py:25-66: timm's
# create_transform with auto_augment='rand-m9-mstd0.5-inc1', bicubic, re_prob=0.25, re_mode='pixel', re_count=1).
# timm is not vendored by the reference: the op list, level maps and RandomErasing restate timm 0.3.2's published
# source; the pixel rules are PIL's (include/ssl4gie_hip.h, tests/randaug_checks.py).
# ------------------------------------------------------------------------------------------------
RANDAUG_OPS = ("AutoContrast", "Equalize", "Invert", "Rotate", "Posterize", "Solarize", "SolarizeAdd", "Color", "Contrast",
               "Brightness", "Sharpness", "ShearX", "ShearY", "TranslateXRel", "TranslateYRel")   # id = position
RANDAUG_SKIP = 255


def randaug_level_args(op, magnitude, negate, inc, size):
    """timm's level functions (auto_augment.py, _MAX_LEVEL = 10) as a pure function of the draws: op int64 [N] (ids of
    RANDAUG_OPS), magnitude float64 [N] in [0, 10], negate bool [N] (_randomly_negate's `random() > 0.5`), inc: the
    'Increasing' variants of Posterize / Solarize / Color / Contrast / Brightness / Sharpness.  Returns arg fp32 [N] — what
    the kernel reads: bits, threshold, addend, blend factor; for the geometric ops degrees, shear or pixels, for the
    record — and matrix float64 [N, 6], PIL's AFFINE coefficients (the identity for the other ops).  float64 in timm's
    order of operations on op's device, no host read-back.  Image.rotate rounds cos and sin to 15 decimals; this does not."""
    lv = magnitude.to(torch.float64) / 10
    neg = lambda v: torch.where(negate, -v, v)
    zero = torch.zeros_like(lv)
    rot = neg(lv * 30.)
    post = torch.trunc(lv * 4)
    sol = torch.trunc(lv * 256)
    if inc:
        post, sol = 4 - post, 256 - sol
    sadd = torch.trunc(lv * 110)
    enh = 1.0 + neg(lv * .9) if inc else lv * 1.8 + 0.1
    shear = neg(lv * 0.3)
    trans = neg(lv * 0.45) * size
    table = torch.stack([zero, zero, zero, rot, post, sol, sadd, enh, enh, enh, enh, shear, shear, trans, trans], dim=1)
    known = (op >= 0) & (op < len(RANDAUG_OPS))
    arg = torch.where(known, table.gather(1, op.clamp(0, len(RANDAUG_OPS) - 1).view(-1, 1)).squeeze(1), zero)
    a = -torch.deg2rad(rot)
    c, s = torch.cos(a), torch.sin(a)
    half = size / 2.0
    is_rot = op == 3
    one = torch.ones_like(lv)
    m2 = (c * -half + s * -half + 0.0) + half     # Image.rotate: the centre through the matrix, then the centre added
    m5 = (-s * -half + c * -half + 0.0) + half
    matrix = torch.stack([torch.where(is_rot, c, one),
                          torch.where(is_rot, s, torch.where(op == 11, shear, zero)),
                          torch.where(is_rot, m2, torch.where(op == 13, trans, zero)),
                          torch.where(is_rot, -s, torch.where(op == 12, shear, zero)),
                          torch.where(is_rot, c, one),
                          torch.where(is_rot, m5, torch.where(op == 14, trans, zero))], dim=1)
    return arg.to(torch.float32), matrix.contiguous()


class RandAugment:
    """timm's rand_augment_transform(config_str, hparams) over the 15 ops of RANDAUG_OPS, drawn on the device:
    config_str 'rand-m9-mstd0.5-inc1' with the keys m (magnitude), n (layers, default 2), mstd (default 0), inc (0 / 1);
    w (weighted choice) raises NotImplementedError.  `size` is the image side (TranslateXRel moves 0.45 level size
    pixels), `mean` gives the fill colour of the geometric ops, min(255, round(255 m)).  Per image and layer: an op
    uniformly from the 15 (with replacement), skipped with probability 0.5, magnitude clip(gauss(m, mstd), 0, 10)."""

    def __init__(self, config_str, size, mean=IMAGENET_MEAN, generator=None):
        parts = str(config_str).split("-")
        if parts[0] != "rand":
            raise ValueError(f"RandAugment takes a 'rand-...' config string, got {config_str!r}")
        self.magnitude, self.layers, self.mstd, self.inc = 10.0, 2, 0.0, 0
        for part in parts[1:]:
            key = part.rstrip("0123456789.")
            val = part[len(key):]
            if not key or not val:
                raise ValueError(f"RandAugment config section {part!r} of {config_str!r} is not a key and a number")
            if key == "w":
                raise NotImplementedError("RandAugment: the weighted op choice ('w') is not built")
            if key == "m":
                self.magnitude = float(int(val))
            elif key == "n":
                self.layers = int(val)
            elif key == "mstd":
                self.mstd = float(val)
            elif key == "inc":
                self.inc = int(bool(int(val)))
            else:
                raise ValueError(f"unknown RandAugment config section {part!r} in {config_str!r}")
        if self.layers < 1 or not 0.0 <= self.magnitude <= 10.0:
            raise ValueError(f"RandAugment needs n >= 1 and 0 <= m <= 10, got {config_str!r}")
        self.size, self.generator = int(size), generator
        self.fill = tuple(min(255, int(round(255 * m))) for m in mean)

    def draw(self, B, device):
        """op uint8 [B, n] (255 = skipped), arg fp32 [B, n], matrix float64 [B, n, 6]; advances the generator.
        Vectorised on the device, no host read-back; timm's random SEQUENCE is not reproduced, its distribution is."""
        n = self.layers
        u = torch.rand(B, n, 3, dtype=torch.float64, device=device, generator=self.generator)
        z = torch.randn(B, n, dtype=torch.float64, device=device, generator=self.generator)
        op = torch.floor(u[..., 0] * len(RANDAUG_OPS)).clamp(max=len(RANDAUG_OPS) - 1).to(torch.int64)
        skip = u[..., 1] > 0.5
        mag = torch.full_like(z, self.magnitude)
        if self.mstd > 0:
            mag = mag + z * self.mstd
        mag = mag.clamp(0.0, 10.0)
        op = torch.where(skip, RANDAUG_SKIP, op)
        arg, matrix = randaug_level_args(op.view(-1), mag.view(-1), (u[..., 2] > 0.5).view(-1), self.inc, self.size)
        return op.to(torch.uint8), arg.view(B, n), matrix.view(B, n, 6)


def erase_boxes(u, H, W, probability=0.5, min_area=0.02, max_area=1 / 3, min_aspect=0.3, max_aspect=None):
    """timm's RandomErasing box choice (max_count = 1) as a pure function of uniforms u [B, 41] in [0, 1): u[:, 0] the
    apply draw (no erase when it exceeds `probability`), then ten tries of (area fraction, log-aspect, top, left); the
    first try with h < H and w < W wins, none: no erase.  float64 on u's device, vectorised, no host read-back.
    Returns int32 [B, 4] = (top, left, h, w), all 0 for no erase."""
    assert u.dim() == 2 and u.shape[1] == 41
    u = u.to(torch.float64)
    B = u.shape[0]
    t = u[:, 1:].view(B, 10, 4)
    l0, l1 = math.log(min_aspect), math.log(max_aspect or 1 / min_aspect)
    target = (min_area + (max_area - min_area) * t[..., 0]) * (H * W)
    aspect = torch.exp(l0 + (l1 - l0) * t[..., 1])
    h = torch.round(torch.sqrt(target * aspect))          # round half to even, as Python's round()
    w = torch.round(torch.sqrt(target / aspect))
    ok = (w < W) & (h < H)
    top = torch.minimum(torch.floor(t[..., 2] * (H - h + 1)), H - h)     # random.randint(0, H - h)
    left = torch.minimum(torch.floor(t[..., 3] * (W - w + 1)), W - w)
    first = torch.argmax(ok.to(torch.uint8), dim=1)
    won = torch.stack([top, left, h, w], dim=2).gather(1, first.view(-1, 1, 1).expand(-1, 1, 4)).squeeze(1)
    apply = ~(u[:, 0] > probability) & ok.any(dim=1)
    return torch.where(apply.unsqueeze(1), won, torch.zeros_like(won)).to(torch.int32)


class RandomErasing:
    """timm.data.RandomErasing(probability, mode, min_area, max_area, min_aspect, max_aspect, max_count=1) on the
    uint8 image that Normalize would read: __call__(img_u8 [B, S, S, 3], seed, mean, std) -> fp32 [B, 3, S, S], the
    normalised batch with one box per erased sample filled with per-element N(0, 1) noise ('pixel'), one N(0, 1) value
    per channel ('rand') or zeros ('const') — one launch of ops.normalize_erase_u8.  max_count > 1 is not built."""

    def __init__(self, probability=0.5, mode="const", min_area=0.02, max_area=1 / 3, min_aspect=0.3, max_aspect=None,
                 max_count=1, generator=None):
        if max_count != 1:
            raise NotImplementedError("RandomErasing: max_count > 1 is not built")
        if mode not in ("const", "rand", "pixel"):
            raise ValueError(f"mode must be 'const', 'rand' or 'pixel', got {mode!r}")
        self.probability, self.mode = float(probability), mode
        self.min_area, self.max_area, self.min_aspect, self.max_aspect = min_area, max_area, min_aspect, max_aspect
        self.generator = generator

    def draw(self, B, H, W, device):
        """box int32 [B, 4] (advances the generator)"""
        u = torch.rand(B, 41, dtype=torch.float64, device=device, generator=self.generator)
        return erase_boxes(u, H, W, self.probability, self.min_area, self.max_area, self.min_aspect, self.max_aspect)

    def __call__(self, img_u8, seed, mean=IMAGENET_MEAN, std=IMAGENET_STD):
        box = self.draw(img_u8.shape[0], img_u8.shape[1], img_u8.shape[2], img_u8.device)
        return ops.normalize_erase_u8(img_u8, box, self.mode, seed, mean, std)


class MAEFinetuneTransform:
    """build_transform(is_train=True) of Models/mae/util/datasets.py:25-48 for DeviceLoader, drawn and computed on the
    bank's device: RandomResizedCropAndInterpolation(input_size, scale, bicubic) + RandomHorizontalFlip
    (RandomResizedCropFlip into 0..255 units) -> ops.quantize_u8 -> the n layers of RandAugment(auto_augment)
    (ops.randaug_layer between two uint8 buffers kept across calls; None: no layers) -> ToTensor + Normalize +
    RandomErasing(re_prob, re_mode) (ops.normalize_erase_u8).  __call__(bank, index) -> fp32 [B, 3, S, S].
    One generator is drawn from in the order crop, RandAugment, erase; the noise seed of call k is
    noise_seed + k 0x9E3779B97F4A7C15 mod 2^64, noise_seed defaulting to the generator's (or torch's) initial seed, which
    the host knows: nothing is read back.  MAEFinetuneTransform.eval(input_size) is the eval transform."""

    _GOLDEN = 0x9E3779B97F4A7C15

    def __init__(self, input_size=224, auto_augment="rand-m9-mstd0.5-inc1", re_prob=0.25, re_mode="pixel", re_count=1,
                 scale=(0.08, 1.0), mean=IMAGENET_MEAN, std=IMAGENET_STD, generator=None, noise_seed=None):
        self.size, self.mean, self.std, self.generator = int(input_size), tuple(mean), tuple(std), generator
        # the crop in 0..255 units: (v / 255 - 0) / (1 / 255)
        self.crop = RandomResizedCropFlip(self.size, scale=scale, interpolation="bicubic", mean=(0.0, 0.0, 0.0),
                                          std=(1.0 / 255.0,) * 3, generator=generator)
        self.randaug = None if auto_augment is None else RandAugment(auto_augment, self.size, mean, generator)
        self.erase = RandomErasing(re_prob, re_mode, max_count=re_count, generator=generator)
        if noise_seed is None:
            noise_seed = generator.initial_seed() if generator is not None else torch.initial_seed()
        self.noise_seed, self.calls = int(noise_seed) & 0xffffffffffffffff, 0
        self.stored = self.offset = None   # set by eval()
        self._bufs = self._workspace = self._eval_box = None

    @classmethod
    def eval(cls, input_size=224, mean=IMAGENET_MEAN, std=IMAGENET_STD):
        """build_transform(is_train=False), datasets.py:50-66: Resize(int(input_size / crop_pct), bicubic) + CenterCrop
        (input_size) + ToTensor + Normalize, crop_pct = 224 / 256 up to input_size 224 and 1 above, for a bank stored
        square at int(input_size / crop_pct), where the Resize is the identity: the centre box at
        int(round((M - S) / 2.)), bit-equal to ops.normalize_u8 of that slice.  Any other stored size raises."""
        t = cls(input_size, auto_augment=None, re_prob=0.0, mean=mean, std=std, noise_seed=0)
        crop_pct = 224 / 256 if t.size <= 224 else 1.0
        t.stored = int(t.size / crop_pct)
        t.offset = int(round((t.stored - t.size) / 2.))
        return t

    def draw(self, B, Hs, Ws, device):
        """(box int32 [B, 4], flip uint8 [B], layers: None or (op uint8 [n, B], arg fp32 [n, B], matrix float64
        [n, B, 6]), erase box int32 [B, 4], noise seed); advances the generator and the call counter"""
        box, flip = self.crop.draw(B, Hs, Ws, device)
        layers = None
        if self.randaug is not None:
            op, arg, matrix = self.randaug.draw(B, device)
            layers = (op.t().contiguous(), arg.t().contiguous(), matrix.transpose(0, 1).contiguous())
        ebox = self.erase.draw(B, self.size, self.size, device)
        seed = (self.noise_seed + self.calls * self._GOLDEN) & 0xffffffffffffffff
        self.calls += 1
        return box, flip, layers, ebox, seed

    def apply(self, bank, index, box, flip, layers, ebox, seed):
        """the launches, on draws that are given"""
        B, S = index.shape[0], self.size
        x = ops.view_sample_u8(bank.images, index, box, flip, S, "bicubic", self.crop.mean, self.crop.std)
        if self._bufs is None or self._bufs[0].shape[0] < B or self._bufs[0].device != x.device:
            self._bufs = [torch.empty(B, S, S, 3, dtype=torch.uint8, device=x.device) for _ in range(2)]
            self._workspace = ops.randaug_layer_workspace(B, x.device)
        cur, nxt = self._bufs[0][:B], self._bufs[1][:B]
        ops.quantize_u8(x, cur)
        if layers is not None:
            for op, arg, matrix in zip(*layers):
                ops.randaug_layer(cur, op, arg, matrix, self.randaug.fill, nxt, self._workspace)
                cur, nxt = nxt, cur
        return ops.normalize_erase_u8(cur, ebox, self.erase.mode, seed, self.mean, self.std)

    def __call__(self, bank, index):
        Hs, Ws = bank.stored_size
        if self.stored is not None:
            if (Hs, Ws) != (self.stored, self.stored):
                raise ValueError(f"MAEFinetuneTransform.eval({self.size}) needs a bank stored at {self.stored} x "
                                 f"{self.stored} (Resize({self.stored}) is then the identity), got {Hs} x {Ws}: pack it "
                                 f"at {self.stored} (tools/pack_images.py --size {self.stored})")
            B = index.shape[0]
            if self._eval_box is None or self._eval_box.device != index.device:
                self._eval_box = torch.tensor([[self.offset, self.offset, self.size, self.size]], dtype=torch.int32,
                                              device=index.device)
            return ops.view_sample_u8(bank.images, index, self._eval_box.expand(B, 4).contiguous(), None, self.size,
                                      "bicubic", self.mean, self.std)
        return self.apply(bank, index, *self.draw(index.shape[0], Hs, Ws, index.device))


class MAELinprobeTransform(RandomResizedCropFlip):
    """transform_train of Models/mae/main_linprobe.py:132-136 for DeviceLoader: util/crop.py's RandomResizedCrop
    (input_size, scale (0.08, 1), bicubic; the one-draw box rule, sampler="tf") + RandomHorizontalFlip + ToTensor +
    Normalize — a weak augmentation, no RandAugment, no erasing.  `MAELinprobeTransform.eval(input_size)` is
    transform_val (:137-141: Resize(256, bicubic) + CenterCrop(224)), which is MAEFinetuneTransform.eval."""

    def __init__(self, input_size=224, scale=(0.08, 1.0), mean=IMAGENET_MEAN, std=IMAGENET_STD, generator=None):
        super().__init__(input_size, scale=scale, interpolation="bicubic", mean=mean, std=std, generator=generator,
                         sampler="tf")

    @staticmethod
    def eval(input_size=224, mean=IMAGENET_MEAN, std=IMAGENET_STD):
        return MAEFinetuneTransform.eval(input_size, mean=mean, std=std)


# ------------------------------------------------------------------------------------------------
# Mixup / CutMix of the MAE fine-tuning recipe (timm.data.Mixup; reference Models/mae/main_finetune.py:221-226)
# ------------------------------------------------------------------------------------------------
def _cutmix_boxes(rs, H, W, lam, minmax, correct_lam):
    """timm's rand_bbox / rand_bbox_minmax + the lambda correction for a vector of lambdas: (y0, y1, x0, x1) int
    arrays and the lambdas that go with them, 1 - area / (H W) when corrected"""
    n = lam.shape[0]
    if minmax is not None:
        ch = rs.randint(int(H * minmax[0]), int(H * minmax[1]), size=n)
        cw = rs.randint(int(W * minmax[0]), int(W * minmax[1]), size=n)
        y0 = rs.randint(0, H - ch)
        x0 = rs.randint(0, W - cw)
        y1, x1 = y0 + ch, x0 + cw
    else:
        ratio = np.sqrt(1.0 - lam.astype(np.float64))
        ch, cw = (H * ratio).astype(np.int64), (W * ratio).astype(np.int64)
        cy, cx = rs.randint(0, H, size=n), rs.randint(0, W, size=n)
        y0, y1 = np.clip(cy - ch // 2, 0, H), np.clip(cy + ch // 2, 0, H)
        x0, x1 = np.clip(cx - cw // 2, 0, W), np.clip(cx + cw // 2, 0, W)
    if correct_lam or minmax is not None:
        lam = 1.0 - ((y1 - y0) * (x1 - x0)) / float(H * W)
    return y0, y1, x0, x1, lam


def mixup_tables(rs, B, H, W, mixup_alpha=1.0, cutmix_alpha=0.0, cutmix_minmax=None, prob=1.0, switch_prob=0.5,
                 mode="batch", correct_lam=True):
    """The per-sample tables of one Mixup call, a pure function of a numpy RandomState (which it advances):
    lam fp32 [B], box int32 [B, 4] = (y0, y1, x0, x1), use_cutmix uint8 [B].  Sample i is mixed with B - 1 - i.
    use_cutmix[i] = 1 copies the partner's box into sample i (lam is then 1 - area / (H W)); an unmixed sample
    (lam = 1) is the empty box, so it comes through bit for bit; use_cutmix[i] = 0 blends with lam[i].  The modes of
    timm differ only in how the tables are filled: `batch` one draw repeated, `elem` one draw per sample, `pair` one
    draw per pair, mirrored (an odd batch's middle sample stays unmixed)."""
    if mode not in ("batch", "pair", "elem"):
        raise ValueError(f"mode must be 'batch', 'pair' or 'elem', got {mode!r}")
    if cutmix_minmax is not None:
        assert len(cutmix_minmax) == 2
        cutmix_alpha = 1.0   # as timm: the box is drawn from the range, lambda follows from its area
    if not (mixup_alpha > 0.0 or cutmix_alpha > 0.0):
        raise ValueError("one of mixup_alpha, cutmix_alpha, cutmix_minmax must be set")
    n = {"batch": 1, "pair": B // 2, "elem": B}[mode]
    on = rs.rand(n) < prob
    if mixup_alpha > 0.0 and cutmix_alpha > 0.0:
        cut = rs.rand(n) < switch_prob
        lam = np.where(cut, rs.beta(cutmix_alpha, cutmix_alpha, size=n), rs.beta(mixup_alpha, mixup_alpha, size=n))
    elif mixup_alpha > 0.0:
        cut = np.zeros(n, dtype=bool)
        lam = rs.beta(mixup_alpha, mixup_alpha, size=n)
    else:
        cut = np.ones(n, dtype=bool)
        lam = rs.beta(cutmix_alpha, cutmix_alpha, size=n)
    lam = np.where(on, lam, 1.0).astype(np.float32)
    y0, y1, x0, x1, lam_box = _cutmix_boxes(rs, H, W, lam, cutmix_minmax, correct_lam)
    cut = cut & on & (lam != 1.0)
    lam = np.where(cut, lam_box, lam).astype(np.float32)
    unmixed = lam == 1.0
    box = np.stack([y0, y1, x0, x1], axis=1).astype(np.int32)
    box[~cut] = 0
    use = (cut | unmixed).astype(np.uint8)   # an unmixed sample: the empty box
    if mode == "batch":
        lam, box, use = np.repeat(lam, B), np.repeat(box, B, axis=0), np.repeat(use, B)
    elif mode == "pair":
        mid = B - 2 * n   # 1 for an odd batch
        lam = np.concatenate([lam, np.ones(mid, np.float32), lam[::-1]])
        box = np.concatenate([box, np.zeros((mid, 4), np.int32), box[::-1]])
        use = np.concatenate([use, np.ones(mid, np.uint8), use[::-1]])
    return np.ascontiguousarray(lam, np.float32), np.ascontiguousarray(box, np.int32), np.ascontiguousarray(use, np.uint8)


def mixup_torch(x, lam, box, use_cutmix):
    """the torch formulation of the image kernel on tensors of any device, out of place: x [B, C, H, W] fp32 and the
    tables of mixup_tables as tensors -> the mixed batch (blend: x.mul(lam).add(x.flip(0).mul(1 - lam)))"""
    B, _, H, W = x.shape
    xf = x.flip(0)
    l4 = lam.to(x.dtype).view(B, 1, 1, 1)
    blend = x.mul(l4).add(xf.mul(1 - l4))
    ys = torch.arange(H, device=x.device).view(1, H, 1)
    xs = torch.arange(W, device=x.device).view(1, 1, W)
    b = box.to(torch.int64)
    inside = ((ys >= b[:, 0].view(B, 1, 1)) & (ys < b[:, 1].view(B, 1, 1)) &
              (xs >= b[:, 2].view(B, 1, 1)) & (xs < b[:, 3].view(B, 1, 1))).unsqueeze(1)
    return torch.where(use_cutmix.view(B, 1, 1, 1) != 0, torch.where(inside, xf, x), blend)


def mixup_target_torch(target, lam, num_classes, smoothing):
    """timm's mixup_target on tensors of any device: fp32 [B, C] = onehot(y) lam + onehot(y.flip(0)) (1 - lam) with
    one-hot values off = smoothing / C and on = 1 - smoothing + off"""
    off = smoothing / num_classes
    on = 1.0 - smoothing + off
    t = target.long().view(-1, 1)
    y1 = torch.full((t.shape[0], num_classes), off, dtype=torch.float32, device=target.device).scatter_(1, t, on)
    y2 = torch.full((t.shape[0], num_classes), off, dtype=torch.float32, device=target.device).scatter_(1, t.flip(0), on)
    l2 = lam.to(torch.float32).view(-1, 1)
    return y1 * l2 + y2 * (1.0 - l2)


class Mixup:
    """timm.data.Mixup with its constructor keywords, for batches that live on the device: `__call__(x, target) ->
    (x, soft_target)` mixes x [B, C, H, W] fp32 IN PLACE (one launch of ops.mixup) and returns fp32 [B, num_classes]
    soft targets (a second small launch).  lambda, the mixup / cutmix choice and the boxes are drawn on the host
    from `rng` (a numpy RandomState; a few numbers per batch, mixup_tables) and reach the device in one small
    non-blocking copy; nothing is read back.  CPU tensors take the torch formulation.  Unlike timm an odd batch is
    accepted: its middle sample is mixed with itself."""

    def __init__(self, mixup_alpha=1., cutmix_alpha=0., cutmix_minmax=None, prob=1.0, switch_prob=0.5, mode="batch",
                 correct_lam=True, label_smoothing=0.1, num_classes=1000, rng=None):
        self.mixup_alpha, self.cutmix_alpha, self.cutmix_minmax = mixup_alpha, cutmix_alpha, cutmix_minmax
        self.mix_prob, self.switch_prob, self.mode, self.correct_lam = prob, switch_prob, mode, correct_lam
        self.label_smoothing, self.num_classes = label_smoothing, num_classes
        self.mixup_enabled = True   # timm's switch: set to False to pass batches through unmixed
        self.rng = rng if rng is not None else np.random.RandomState()
        self._staging = []          # [pinned buffer, event of its last copy] x 2, used in turn
        self._turn = 0
        mixup_tables(np.random.RandomState(0), 2, 8, 8, mixup_alpha, cutmix_alpha, cutmix_minmax, prob, switch_prob,
                     mode, correct_lam)   # validates the keywords

    def draw(self, B, H, W):
        """the numpy tables of the next call (advances `rng`)"""
        return mixup_tables(self.rng, B, H, W, self.mixup_alpha, self.cutmix_alpha, self.cutmix_minmax,
                            self.mix_prob if self.mixup_enabled else 0.0, self.switch_prob, self.mode, self.correct_lam)

    def _upload(self, lam, box, use, device):
        """lam | box | use_cutmix through one pinned staging buffer and one non-blocking copy"""
        B = lam.shape[0]
        nbytes = 21 * B
        if len(self._staging) < 2 or self._staging[0][0].numel() < nbytes:
            self._staging = [[torch.empty(max(nbytes, 21 * 256), dtype=torch.uint8).pin_memory(), None] for _ in range(2)]
        slot = self._staging[self._turn]
        self._turn ^= 1
        if slot[1] is not None:
            slot[1].synchronize()   # the copy issued two calls ago: long done
        host = slot[0].numpy()
        host[:4 * B] = lam.view(np.uint8)
        host[4 * B:20 * B] = box.reshape(-1).view(np.uint8)
        host[20 * B:nbytes] = use
        dev = slot[0][:nbytes].to(device, non_blocking=True)
        slot[1] = torch.cuda.Event()
        slot[1].record()
        return dev[:4 * B].view(torch.float32), dev[4 * B:20 * B].view(torch.int32).view(B, 4), dev[20 * B:]

    def apply_tables(self, x, target, lam, box, use_cutmix):
        """mix with given tables (tensors on x's device)"""
        if x.is_cuda:
            ops.mixup(x, lam, box, use_cutmix)
            return x, ops.mixup_target(target, lam, self.num_classes, self.label_smoothing)
        x.copy_(mixup_torch(x, lam, box, use_cutmix))
        return x, mixup_target_torch(target, lam, self.num_classes, self.label_smoothing)

    def __call__(self, x, target):
        B, _, H, W = x.shape
        lam, box, use = self.draw(B, H, W)
        if x.is_cuda:
            tabs = self._upload(lam, box, use, x.device)
        else:
            tabs = (torch.from_numpy(lam), torch.from_numpy(box), torch.from_numpy(use))
        return self.apply_tables(x, target, *tabs)
