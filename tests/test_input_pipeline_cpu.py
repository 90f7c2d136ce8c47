"""CPU: the host / torch-op side of the on-device input pipeline (ssl4gie_amd.data) — the crop-box draw against a
scalar restatement of RandomResizedCrop.get_params, the loader's batching over torch's own samplers — and the C ABI
declaration of the view sampler."""
import math
import os
import re

import pytest
import torch

from conftest import ROOT


def get_params_scalar(u, height, width, scale, ratio):
    """torchvision.transforms.RandomResizedCrop.get_params, statement for statement, with its random draws
    replaced by the uniforms u[10][4]: uniform_(a, b) = a + u (b - a), randint(0, n) = floor(u n).  Returns
    (top, left, height, width, the try that won — 10 for the fallback)"""
    area = height * width
    log_ratio = (math.log(ratio[0]), math.log(ratio[1]))
    for t in range(10):
        target_area = area * (scale[0] + u[t][0] * (scale[1] - scale[0]))
        aspect_ratio = math.exp(log_ratio[0] + u[t][1] * (log_ratio[1] - log_ratio[0]))
        w = int(round(math.sqrt(target_area * aspect_ratio)))
        h = int(round(math.sqrt(target_area / aspect_ratio)))
        if 0 < w <= width and 0 < h <= height:
            i = int(math.floor(u[t][2] * (height - h + 1)))
            j = int(math.floor(u[t][3] * (width - w + 1)))
            return i, j, h, w, t
    in_ratio = float(width) / float(height)
    if in_ratio < min(ratio):
        w = width
        h = int(round(w / min(ratio)))
    elif in_ratio > max(ratio):
        h = height
        w = int(round(h * max(ratio)))
    else:
        w = width
        h = height
    i = (height - h) // 2
    j = (width - w) // 2
    return i, j, h, w, 10


RATIO = (3.0 / 4.0, 4.0 / 3.0)


@pytest.mark.parametrize("Hs,Ws,scale", [(96, 81, (0.2, 1.0)), (96, 81, (0.9, 1.0)), (96, 30, (0.2, 1.0)),
                                         (30, 96, (0.2, 1.0))])
def test_rrc_boxes_equal_get_params_integer_for_integer(Hs, Ws, scale):
    from ssl4gie_amd.data import rrc_boxes
    B = 4096
    u = torch.rand(B, 10, 4, dtype=torch.float64, generator=torch.Generator().manual_seed(1234))
    got = rrc_boxes(u, Hs, Ws, scale, RATIO)
    assert got.dtype == torch.int32 and tuple(got.shape) == (B, 4)
    ul = u.tolist()
    rows = [get_params_scalar(ul[b], Hs, Ws, scale, RATIO) for b in range(B)]
    want = torch.tensor([r[:4] for r in rows], dtype=torch.int32)
    assert torch.equal(got, want), (got != want).any(dim=1).nonzero()[:5]
    top, left, h, w = got.unbind(1)
    assert bool(((h >= 1) & (w >= 1) & (top >= 0) & (left >= 0) & (top + h <= Hs) & (left + w <= Ws)).all())
    # the branch each case is there for
    tries = [r[4] for r in rows]
    if (Hs, Ws) == (96, 81):
        later = sum(1 for t in tries if 0 < t < 10)
        assert later > (B // 4 if scale[0] == 0.9 else 0)        # at scale >= 0.9 most first tries are rejected
    else:
        fb = [r[:4] for r in rows if r[4] == 10]
        assert len(fb) > B // 50 and any(t < 10 for t in tries)
        assert set(fb) == {(28, 0, 40, 30) if Hs == 96 else (0, 28, 30, 40)}


class _StubTransform:
    """stands in for RandomResizedCropFlip on CPU tensors: the 'image' is the index itself"""

    def __init__(self, views=1):
        self.views = views

    def __call__(self, bank, index):
        one = bank.images[index][:, 0, 0, 0].to(torch.float32)
        return one if self.views == 1 else [one.clone() for _ in range(self.views)]


def _cpu_bank(n, labels=True):
    from ssl4gie_amd.data import DeviceImageBank
    img = torch.zeros(n, 2, 2, 3, dtype=torch.uint8)
    img[:, 0, 0, 0] = torch.arange(n, dtype=torch.uint8)
    return DeviceImageBank(img, labels=(torch.arange(n) % 5) if labels else None)


def test_device_loader_batches_over_torch_samplers_cpu():
    from torch.utils.data import DistributedSampler, SequentialSampler
    from ssl4gie_amd.data import DeviceImageBank, DeviceLoader
    n, bs = 37, 4
    bank = _cpu_bank(n)
    assert len(bank) == n and bank[5] == (5, 0) and bank[7] == (7, 2) and bank.stored_size == (2, 2)
    with pytest.raises(IndexError):
        bank[n]
    with pytest.raises(ValueError):
        DeviceImageBank(torch.zeros(3, 2, 2, 3))          # not uint8
    assert _cpu_bank(4, labels=False)[3] == (3, 0)
    # plain sequential sampler, both drop_last settings
    seq = DeviceLoader(bank, bs, sampler=SequentialSampler(bank), drop_last=True, transform=_StubTransform())
    assert len(seq) == n // bs
    got = list(seq)
    assert len(got) == len(seq) and all(s.shape == (bs,) and l.shape == (bs,) for s, l in got)
    assert torch.equal(torch.cat([s for s, _ in got]).long(), torch.arange(n - n % bs))
    assert torch.equal(torch.cat([l for _, l in got]), torch.arange(n - n % bs) % 5)
    keep = DeviceLoader(bank, bs, sampler=SequentialSampler(bank), drop_last=False, transform=_StubTransform())
    assert len(keep) == (n + bs - 1) // bs and len(list(keep)) == len(keep) and list(keep)[-1][0].shape == (n % bs,)
    # the default sampler is a RandomSampler over the bank
    assert sorted(int(v) for s, _ in DeviceLoader(bank, 1, transform=_StubTransform()) for v in s) == list(range(n))
    # torch's DistributedSampler at 2 ranks: every index exactly once per epoch, up to its padding
    loaders = [DeviceLoader(bank, bs, sampler=DistributedSampler(bank, num_replicas=2, rank=r, shuffle=True, seed=3),
                            drop_last=False, transform=_StubTransform()) for r in range(2)]
    orders = {}
    for epoch in (0, 1):
        seen = []
        for ld in loaders:
            ld.sampler.set_epoch(epoch)
            assert len(ld) == math.ceil(math.ceil(n / 2) / bs)
            mine = [int(v) for s, _ in ld for v in s]
            assert len(mine) == math.ceil(n / 2)
            seen += mine
        assert sorted(set(seen)) == list(range(n)) and len(seen) == 2 * math.ceil(n / 2)
        assert len(seen) - len(set(seen)) == 2 * math.ceil(n / 2) - n          # only the padding repeats
        orders[epoch] = seen
    assert orders[0] != orders[1]                                              # set_epoch reshuffles
    # a two-view transform yields a list, as the MoCo loop indexes it (images[0], images[1])
    two = DeviceLoader(bank, bs, sampler=SequentialSampler(bank), transform=_StubTransform(views=2))
    images, labels = next(iter(two))
    assert isinstance(images, list) and len(images) == 2 and torch.equal(images[0], images[1]) and labels.shape == (bs,)


def test_transform_and_ops_refuse_what_the_kernel_cannot_take_cpu():
    from ssl4gie_amd import ops
    from ssl4gie_amd.data import RandomResizedCropFlip
    bank = _cpu_bank(4)
    idx = torch.zeros(2, dtype=torch.int64)
    box = torch.tensor([[0, 0, 2, 2]] * 2, dtype=torch.int32)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.view_sample_u8(bank.images, idx, box, None, 8)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        RandomResizedCropFlip(8)(bank, idx)
    with pytest.raises(ValueError):
        RandomResizedCropFlip(8, interpolation="nearest")
    with pytest.raises(ValueError):
        RandomResizedCropFlip(30)
    t = RandomResizedCropFlip(8, generator=torch.Generator().manual_seed(5))
    b1, f1 = t.draw(64, 96, 81, torch.device("cpu"))
    b2, f2 = RandomResizedCropFlip(8, generator=torch.Generator().manual_seed(5)).draw(64, 96, 81, torch.device("cpu"))
    assert torch.equal(b1, b2) and torch.equal(f1, f2) and f1.dtype == torch.uint8 and 0 < int(f1.sum()) < 64
    b3, _ = t.draw(64, 96, 81, torch.device("cpu"))
    assert not torch.equal(b1, b3)                                             # the generator advances


def test_from_npy_is_chunked_and_equal(tmp_path):
    import numpy as np
    from ssl4gie_amd.data import DeviceImageBank
    arr = np.random.default_rng(0).integers(0, 256, size=(11, 6, 5, 3), dtype=np.uint8)
    np.save(tmp_path / "bank.npy", arr)
    np.save(tmp_path / "labels.npy", np.arange(11) % 3)
    bank = DeviceImageBank.from_npy(str(tmp_path / "bank.npy"), "cpu", labels=str(tmp_path / "labels.npy"),
                                    chunk_bytes=2 * 6 * 5 * 3)              # 2 images per chunk, a ragged last one
    assert torch.equal(bank.images, torch.from_numpy(arr)) and bank[4] == (4, 1)
    assert torch.equal(DeviceImageBank.from_uint8(arr, "cpu").images, bank.images)


def test_header_declares_and_lib_binds_the_view_sampler():
    from ssl4gie_amd import _lib
    txt = open(os.path.join(ROOT, "include", "ssl4gie_hip.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    declared = set(re.findall(r"\b(ssl4gie_[a-z0-9_]+)\s*\(", txt))
    assert "ssl4gie_view_sample_u8" in declared and "ssl4gie_view_sample_u8" in _lib.PROTOTYPES
    assert re.search(r"#define\s+SSL4GIE_FILTER_BILINEAR\s+0\b", txt) and re.search(r"#define\s+SSL4GIE_FILTER_BICUBIC\s+1\b", txt)
    assert (_lib.FILTER_BILINEAR, _lib.FILTER_BICUBIC) == (0, 1)
    assert _lib.ABI_VERSION == 13 and _lib.load().ssl4gie_abi_version() == 13
    # host-checkable arguments are refused before anything is launched (no GPU needed: SSL4GIE_EARG)
    import ctypes as C
    L = _lib.load()
    m, s, z = (C.c_float * 3)(0, 0, 0), (C.c_float * 3)(1, 1, 1), (C.c_float * 3)(1, 0, 1)
    p = 4096  # any non-null value: never dereferenced on these paths
    assert L.ssl4gie_view_sample_u8(p, 3, 96, 81, p, p, None, p, 2, 30, 1, m, s, None) == 1000      # S % 4
    assert L.ssl4gie_view_sample_u8(p, 3, 96, 81, p, p, None, p, 2, 32, 1, m, z, None) == 1000      # std = 0
    assert L.ssl4gie_view_sample_u8(p, 3, 96, 81, p, p, None, p, 2, 32, 7, m, s, None) == 1000      # filter
    assert L.ssl4gie_view_sample_u8(None, 3, 96, 81, p, p, None, p, 2, 32, 1, m, s, None) == 1000   # null bank
    assert L.ssl4gie_view_sample_u8(p, 3, 8192, 8192, p, p, None, p, 2, 224, 1, m, s, None) == 1000  # LDS plan


def test_pack_images_tool_writes_a_loadable_bank(tmp_path):
    import sys
    import numpy as np
    from PIL import Image
    from ssl4gie_amd.data import DeviceImageBank
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import pack_images
    rng = np.random.default_rng(0)
    src = {}
    for cls, names in (("b_polyp", ("2.png", "1.png")), ("a_normal", ("x.png",))):
        os.makedirs(tmp_path / "data" / cls)
        for nm in names:
            src[f"{cls}/{nm}"] = rng.integers(0, 256, size=(12, 10, 3), dtype=np.uint8)
            Image.fromarray(src[f"{cls}/{nm}"]).save(tmp_path / "data" / cls / nm)
    out = str(tmp_path / "bank")
    assert pack_images.pack(str(tmp_path / "data"), out, 12, 10) == 3
    files = open(out + ".files.txt").read().split()
    assert files == ["a_normal/x.png", "b_polyp/1.png", "b_polyp/2.png"]        # ImageFolder's order
    bank = DeviceImageBank.from_npy(out + ".npy", "cpu", labels=out + ".labels.npy")
    assert len(bank) == 3 and bank.stored_size == (12, 10) and [bank[i][1] for i in range(3)] == [0, 1, 1]
    for k, f in enumerate(files):                                               # stored size == source size: verbatim
        assert np.array_equal(bank.images[k].numpy(), src[f])
    assert pack_images.pack(str(tmp_path / "data"), out + "_8", 8, 8, center_crop=True) == 3
    assert np.load(out + "_8.npy").shape == (3, 8, 8, 3)
