"""CPU: the host side of the detection input pipeline (ssl4gie_amd.data.RaggedImageBank, DetectionTransform,
DetectionLoader), the ragged packer, and the C ABI declarations of the three entry points."""
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT


def images(shapes, seed=0):
    rng = np.random.default_rng(seed)
    return [rng.integers(0, 256, size=(h, w, 3), dtype=np.uint8) for h, w in shapes]


SHAPES = ((13, 20), (40, 15), (33, 33), (16, 16), (50, 70))
BOXES = ([[1, 2, 3, 4]], np.zeros((0, 4)), [[0, 0, 5, 5], [1, 1, 2, 2], [3, 3, 9, 9]], [], [[2.5, 3.5, 4.5, 5.5]])


def bank():
    from ssl4gie_amd.data import RaggedImageBank
    return RaggedImageBank.from_arrays(images(SHAPES), BOXES, "cpu")


def test_bank_layout():
    b, imgs = bank(), images(SHAPES)
    assert len(b) == 5 and b[3] == (3, 0) and b.device.type == "cpu"
    with pytest.raises(IndexError):
        b[5]
    assert b.pixels.dtype == torch.uint8 and b.pixels.dim() == 1
    assert b.sizes.dtype == torch.int32 and b.sizes.tolist() == [list(s) for s in SHAPES] and b.sizes_host == list(SHAPES)
    assert b.offsets.dtype == torch.int64 and all(o % 16 == 0 for o in b.offsets.tolist())
    want, at = [], 0
    for h, w in SHAPES:
        want.append(at)
        at += (h * w * 3 + 15) // 16 * 16
    assert b.offsets.tolist() == want and b.pixels.numel() == at
    for k, im in enumerate(imgs):
        assert np.array_equal(b.image(k).numpy(), im)
    assert b.boxes.dtype == torch.float32 and tuple(b.boxes.shape) == (5, 4)
    assert b.box_offsets.dtype == torch.int64 and b.box_offsets.tolist() == [0, 1, 1, 4, 4, 5] == b.box_offsets_host
    assert b.box_labels.dtype == torch.int64 and b.box_labels.tolist() == [1] * 5
    assert b.max_hw == (50, 70) and b.max_pixels == 3500
    # torch's samplers work on it unchanged
    s = torch.utils.data.DistributedSampler(b, num_replicas=2, rank=1, shuffle=True)
    s.set_epoch(3)
    assert len(list(s)) == 3


def test_bank_refusals():
    from ssl4gie_amd.data import RaggedImageBank as R
    imgs = images(SHAPES)
    with pytest.raises(ValueError, match="13"):
        R.from_arrays(images(((12, 40),)), [[]], "cpu")
    with pytest.raises(ValueError):
        R.from_arrays([imgs[0].astype(np.int16)], [[]], "cpu")
    with pytest.raises(ValueError):
        R.from_arrays([imgs[4][:, ::2]], [[]], "cpu")             # non-contiguous
    with pytest.raises(ValueError):
        R.from_arrays(imgs, BOXES[:4], "cpu")                     # one box array short
    with pytest.raises(ValueError):
        R.from_arrays(imgs[:1], [[[1, 2, 3]]], "cpu")             # [k, 3]
    with pytest.raises(ValueError):
        R.from_arrays([], [], "cpu")
    b = bank()
    ok = (b.pixels, b.sizes, b.boxes, b.box_offsets)
    R(*ok)
    bad = [
        (b.pixels.to(torch.int8), b.sizes, b.boxes, b.box_offsets),
        (torch.cat([b.pixels, b.pixels])[::2], b.sizes, b.boxes, b.box_offsets),
        (b.pixels[:-16], b.sizes, b.boxes, b.box_offsets),
        (b.pixels, b.sizes.to(torch.int64), b.boxes, b.box_offsets),
        (b.pixels, b.sizes.view(-1), b.boxes, b.box_offsets),
        (b.pixels, b.sizes, b.boxes.double(), b.box_offsets),
        (b.pixels, b.sizes, b.boxes[:, :3], b.box_offsets),
        (b.pixels, b.sizes, b.boxes, b.box_offsets.to(torch.int32)),
        (b.pixels, b.sizes, b.boxes, b.box_offsets[:-1]),
        (b.pixels, b.sizes, b.boxes[:4], b.box_offsets),          # the count does not match box_offsets[-1]
        (b.pixels, b.sizes, b.boxes, b.box_offsets.flip(0)),
    ]
    for args in bad:
        with pytest.raises(ValueError):
            R(*args)
    with pytest.raises(ValueError):
        R(*ok, torch.ones(4, dtype=torch.int64))
    with pytest.raises(ValueError):
        R(*ok, torch.ones(5, dtype=torch.int32))


def test_packer_round_trip(tmp_path):
    from PIL import Image
    from ssl4gie_amd.data import RaggedImageBank
    folder = tmp_path / "images"
    folder.mkdir()
    names = ["b_02.png", "a_10.png", "c_01.png"]
    shapes = {"b_02.png": (20, 31), "a_10.png": (45, 13), "c_01.png": (16, 16)}
    table, pix = {}, {}
    rng = np.random.default_rng(4)
    for k, name in enumerate(names):
        h, w = shapes[name]
        pix[name] = rng.integers(0, 256, size=(h, w, 3), dtype=np.uint8)
        Image.fromarray(pix[name]).save(folder / name)
        table[name[:-4]] = {"height": h, "width": w, "bbox": [
            {"label": "polyp", "xmin": 1 + j, "ymin": 2 + j, "xmax": 8 + j, "ymax": 9 + j} for j in range(k)]}
    (tmp_path / "bounding-boxes.json").write_text(json.dumps(table))
    out = str(tmp_path / "det")
    subprocess.run([sys.executable, os.path.join(ROOT, "tools", "pack_images.py"), str(folder), "--ragged", "--boxes",
                    str(tmp_path / "bounding-boxes.json"), "--out", out], check=True, capture_output=True)
    b = RaggedImageBank.from_npy(out, "cpu", chunk_bytes=1000)      # several chunks
    order = sorted(names)                                            # sorted-glob order
    assert open(out + ".files.txt").read().split() == order and len(b) == 3
    for k, name in enumerate(order):
        assert np.array_equal(b.image(k).numpy(), pix[name]) and b.sizes_host[k] == shapes[name]
    assert b.box_offsets_host == [0, 1, 1, 3]                        # a_10 was written second (1 box), b_02 first (0), c_01 third (2)
    assert b.boxes.tolist() == [[1, 2, 8, 9], [1, 2, 8, 9], [2, 3, 9, 10]]
    assert b.box_labels.tolist() == [1, 1, 1]
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "pack_images.py"), str(folder), "--ragged", "--out", out],
                       capture_output=True)
    assert r.returncode != 0


def test_draw_shapes_dtypes_and_seed():
    from ssl4gie_amd.data import DetectionTransform
    t = DetectionTransform(64, generator=torch.Generator().manual_seed(7))
    factors, order, sigma, geom = t.draw(500, "cpu")
    assert factors.dtype == torch.float32 and tuple(factors.shape) == (500, 4)
    assert order.dtype == torch.uint8 and tuple(order.shape) == (500, 4)
    assert sigma.dtype == torch.float32 and tuple(sigma.shape) == (500,)
    assert geom.dtype == torch.uint8 and tuple(geom.shape) == (500,)
    assert sorted(set(geom.tolist())) == list(range(8))              # every combination of (r, h, v) is drawn
    assert all(sorted(o) == [0, 1, 2, 3] for o in order.tolist())
    assert 0.001 <= float(sigma.min()) and float(sigma.max()) <= 2.0
    lo, hi = torch.tensor([0.6, 0.5, 0.75, -0.01]), torch.tensor([1.4, 1.5, 1.25, 0.01])
    assert bool(((factors >= lo) & (factors <= hi)).all())
    again = DetectionTransform(64, generator=torch.Generator().manual_seed(7)).draw(500, "cpu")
    assert all(torch.equal(a, b) for a, b in zip((factors, order, sigma, geom), again))
    other = DetectionTransform(64, generator=torch.Generator().manual_seed(8)).draw(500, "cpu")
    assert not torch.equal(geom, other[3])


@pytest.mark.parametrize("off", ("rotate", "hflip", "vflip"))
def test_a_switched_off_decision_is_never_drawn(off):
    from ssl4gie_amd.data import DetectionTransform
    bit = {"hflip": 1, "vflip": 2, "rotate": 4}[off]
    t = DetectionTransform(64, generator=torch.Generator().manual_seed(1), **{off: False})
    geom = t.draw(2000, "cpu")[3]
    assert int((geom & bit).sum()) == 0 and len(set(geom.tolist())) == 4


def test_eval_transform_draws_nothing():
    from ssl4gie_amd.data import DetectionTransform
    factors, order, sigma, geom = DetectionTransform.eval(64).draw(50, "cpu")
    assert factors is None and order is None and sigma is None and geom.tolist() == [0] * 50


def test_transform_refusals():
    from ssl4gie_amd.data import DetectionLoader, DetectionTransform, DeviceImageBank
    with pytest.raises(ValueError):
        DetectionTransform(62)
    with pytest.raises(ValueError):
        DetectionTransform(64, std=(1.0, 0.0, 1.0))
    with pytest.raises(ValueError):
        DetectionTransform(64, blur_sigma=(0.0, 2.0))
    b = bank()                                                       # largest side 70
    DetectionTransform(36).check(b)
    with pytest.raises(ValueError, match="2 x fixed_size"):
        DetectionTransform(32).check(b)
    with pytest.raises(ValueError, match="2 x fixed_size"):
        DetectionLoader(b, 2, transform=DetectionTransform.eval(32))
    with pytest.raises(TypeError):
        DetectionTransform(64).check(DeviceImageBank(torch.zeros(1, 16, 16, 3, dtype=torch.uint8)))
    with pytest.raises(ValueError):
        DetectionLoader(b, 0)


def test_loader_length_and_drop_last():
    from ssl4gie_amd.data import DetectionLoader, DetectionTransform
    b = bank()
    t = DetectionTransform(64)
    assert len(DetectionLoader(b, 2, transform=t)) == 2
    assert len(DetectionLoader(b, 2, drop_last=False, transform=t)) == 3
    assert len(DetectionLoader(b, 5, transform=t)) == 1 and len(DetectionLoader(b, 6, transform=t)) == 0
    s = torch.utils.data.DistributedSampler(b, num_replicas=2, rank=0, shuffle=False)
    loader = DetectionLoader(b, 2, sampler=s, transform=t)
    assert len(loader) == 1 and loader.sampler is s


NEW_SYMBOLS = ("ssl4gie_det_color_workspace_bytes", "ssl4gie_det_color", "ssl4gie_det_geometry", "ssl4gie_det_boxes")


def test_new_symbols_declared_bound_and_resolvable():
    from ssl4gie_amd import _lib, ops
    txt = open(os.path.join(ROOT, "include", "ssl4gie_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    lib = _lib.load()
    for name in NEW_SYMBOLS:
        assert re.search(r"\b" + name + r"\s*\(", code), name
        assert name in _lib.PROTOTYPES and hasattr(lib, name)
        decl = re.search(r"\b" + name + r"\s*\(([^;]*)\)\s*;", code).group(1)
        assert len([a for a in decl.split(",") if a.strip()]) == len(_lib.PROTOTYPES[name][1]), name
    assert _lib.ABI_VERSION == 13 and lib.ssl4gie_abi_version() == 13
    assert lib.ssl4gie_det_color_workspace_bytes(0) == 0 and lib.ssl4gie_det_color_workspace_bytes(4) == 4 * 64 * 4
    # the declarations cite the reference lines they replace
    block = txt[txt.index("The detection loaders (Object_detection"):txt.index("size_t ssl4gie_det_color_workspace_bytes")]
    for cite in ("dataloaders.py:75-112", "dataset.py:38-113", "dataloaders.py:77-80", "dataset.py:50-52", "dataset.py:53-61"):
        assert cite in block, cite
    for fn in ("det_color", "det_geometry", "det_boxes"):
        assert callable(getattr(ops, fn))


def test_ops_refuse_host_tensors():
    from ssl4gie_amd import ops
    b = bank()
    with pytest.raises(RuntimeError, match="HIP device"):
        ops.det_geometry(b.pixels, b.offsets, b.sizes, torch.zeros(1, dtype=torch.int64), None, 64)
