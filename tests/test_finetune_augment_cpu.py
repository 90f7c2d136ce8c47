"""CPU: the host / torch-op side of the finetune augmentation (ssl4gie_amd.data.affine_matrices, FinetuneAugment,
DeviceImageBank targets, tools/pack_images.py --targets) and the C ABI declarations of ssl4gie_color_augment_ft and
ssl4gie_paired_warp with the arguments they refuse before any launch."""
import ctypes as C
import math
import os
import re
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT

import warp_checks as wc

CPU = torch.device("cpu")
IDENTITY = [1.0, 0.0, 0.0, 0.0, 1.0, 0.0]


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _forward_matrix(angle, tx, ty, scale, shear):
    """T * C * RSS * C^-1 with centre 0, from the docstring of torchvision's _get_inverse_affine_matrix:
    RSS = [[cos(a), -sin(a)], [sin(a), cos(a)]] * scale * [[1, -tan(sx)], [0, 1]] (shear along x alone)"""
    a, s = math.radians(angle), math.radians(shear)
    rot = np.array([[math.cos(a), -math.sin(a)], [math.sin(a), math.cos(a)]])
    m = np.eye(3)
    m[:2, :2] = scale * rot @ np.array([[1.0, -math.tan(s)], [0.0, 1.0]])
    m[:2, 2] = (tx, ty)
    return m


def test_affine_matrices_invert_the_forward_map():
    from ssl4gie_amd.data import affine_matrices
    rng = np.random.default_rng(0)
    B = 256
    angle, shear = rng.uniform(-180, 180, B), rng.uniform(-22.5, 22.5, B)
    t, scale = rng.uniform(-28, 28, (B, 2)), rng.uniform(0.5, 1.5, B)
    args = tuple(torch.from_numpy(v) for v in (angle, t, scale, shear))
    m64 = affine_matrices(*args, dtype=torch.float64)
    m32 = affine_matrices(*args)
    assert m32.dtype == torch.float32 and tuple(m32.shape) == (B, 6) and m32.is_contiguous()
    assert torch.equal(m32, m64.to(torch.float32))
    worst = 0.0
    for b in range(B):
        inv = np.eye(3)
        inv[:2] = m64[b].numpy().reshape(2, 3)
        worst = max(worst, float(np.abs(inv @ _forward_matrix(angle[b], t[b, 0], t[b, 1], scale[b], shear[b]) - np.eye(3)).max()))
        assert np.abs(m64[b].numpy() - np.array(wc.inverse_affine(angle[b], t[b, 0], t[b, 1], scale[b], shear[b]))).max() <= 1e-12
    assert worst <= 1e-12, worst


def test_affine_matrices_special_values():
    from ssl4gie_amd.data import affine_matrices
    f64 = lambda *v: torch.tensor(v, dtype=torch.float64)
    assert affine_matrices(f64(0.0)).tolist() == [IDENTITY]
    assert affine_matrices(f64(0.0), f64(0.0, 0.0).view(1, 2), f64(1.0), f64(0.0)).tolist() == [IDENTITY]
    m = affine_matrices(f64(90.0, -90.0, 180.0), dtype=torch.float64)
    want = f64([0, 1, 0, -1, 0, 0], [0, -1, 0, 1, 0, 0], [-1, 0, 0, 0, -1, 0])        # signed permutations
    assert float((m - want).abs().max()) <= 1e-12
    # the translation enters through the inverse: a shift of the image by (+3, -2) reads the source at (-3, +2)
    assert affine_matrices(f64(0.0), f64(3.0, -2.0).view(1, 2)).tolist() == [[1.0, 0.0, -3.0, 0.0, 1.0, 2.0]]
    assert affine_matrices(f64(0.0), None, f64(2.0)).tolist() == [[0.5, 0.0, 0.0, 0.0, 0.5, 0.0]]
    # TF.rotate(angle) is affine(-angle): the two are each other's inverse
    a, b = affine_matrices(f64(33.0), dtype=torch.float64)[0], affine_matrices(f64(-33.0), dtype=torch.float64)[0]
    prod = a.view(2, 3)[:, :2] @ b.view(2, 3)[:, :2]
    assert float((prod - torch.eye(2, dtype=torch.float64)).abs().max()) <= 1e-12


def test_draw_is_seeded_and_the_generator_advances():
    from ssl4gie_amd.data import FinetuneAugment
    t = FinetuneAugment.segmentation(generator=_gen(5))
    a = t.draw(64, CPU)
    b = FinetuneAugment.segmentation(generator=_gen(5)).draw(64, CPU)
    assert len(a) == 6 and all(torch.equal(p, q) for p, q in zip(a, b))
    c = t.draw(64, CPU)
    assert all(not torch.equal(p, q) for k, (p, q) in enumerate(zip(a, c)) if k != 2)      # (the flags are all 0)
    factors, order, flags, sigma, flip, matrix = a
    assert factors.dtype == torch.float32 and tuple(factors.shape) == (64, 4) and factors.is_contiguous()
    assert order.dtype == torch.uint8 and tuple(order.shape) == (64, 4) and order.is_contiguous()
    assert flags.dtype == torch.uint8 and tuple(flags.shape) == (64,) and not bool(flags.any())
    assert sigma.dtype == torch.float32 and tuple(sigma.shape) == (64,)
    assert flip.dtype == torch.uint8 and tuple(flip.shape) == (64,) and flip.is_contiguous()
    assert matrix.dtype == torch.float32 and tuple(matrix.shape) == (64, 6) and matrix.is_contiguous()


def test_draw_follows_the_reference_ranges():
    """Binary_segmentation/Data/dataloaders.py:62-71 and dataset.py:46-63: every parameter inside its range and
    spread over it; the jitter is never skipped; each flip about half of the time, independently"""
    from ssl4gie_amd.data import FinetuneAugment
    B, S = 4096, 224
    t = FinetuneAugment.segmentation(generator=_gen(1))
    assert t.color.ranges() == [(0.6, 1.4), (0.5, 1.5), (0.75, 1.25), (-0.01, 0.01)] and t.fill == (-1.0, -1.0, -1.0)
    factors, order, flags, sigma, flip, matrix = t.draw(B, CPU)
    assert all(sorted(r) == [0, 1, 2, 3] for r in order.tolist())                       # jitter always on
    assert len({tuple(r) for r in order.tolist()}) == 24
    f32 = lambda v: torch.tensor(v, dtype=torch.float32)

    def inside_and_spread(col, lo, hi):
        assert bool((col >= f32(lo)).all()) and bool((col <= f32(hi)).all())
        assert float(col.min()) < lo + 0.02 * (hi - lo) and float(col.max()) > hi - 0.02 * (hi - lo)
        assert abs(float(col.double().mean()) - 0.5 * (lo + hi)) < 0.02 * (hi - lo)

    for k, (lo, hi) in enumerate(t.color.ranges()):
        inside_and_spread(factors[:, k], lo, hi)
    inside_and_spread(sigma, 0.001, 2.0)
    h, v = (flip & 1).float(), ((flip & 2) >> 1).float()
    assert int(flip.max()) <= 3 and 0.46 < float(h.mean()) < 0.54 and 0.46 < float(v.mean()) < 0.54
    assert 0.21 < float((h * v).mean()) < 0.29                                          # independent
    # the matrix back to its parameters: M = [d, -b, ., -c, a, .] / scale with a = cos(rot), c = sin(rot),
    # b = -cos(rot) tan(sx) - sin(rot)
    m = matrix.double()
    scale = 1.0 / torch.sqrt(m[:, 3] ** 2 + m[:, 4] ** 2)
    angle = torch.rad2deg(torch.atan2(-m[:, 3], m[:, 4]))
    lin = torch.stack([m[:, 0], m[:, 1], m[:, 3], m[:, 4]], dim=1).view(B, 2, 2)
    shift = -torch.linalg.solve(lin, torch.stack([m[:, 2], m[:, 5]], dim=1))            # (tx, ty)
    rot = torch.deg2rad(angle)
    shear = torch.rad2deg(torch.atan((m[:, 1] * scale - torch.sin(rot)) / torch.cos(rot)))
    inside_and_spread(angle.float(), -180.0, 180.0)
    inside_and_spread(scale.float(), 0.5, 1.5)
    inside_and_spread(shift[:, 0].float(), -S / 8.0, S / 8.0)
    inside_and_spread(shift[:, 1].float(), -S / 8.0, S / 8.0)
    ok = torch.cos(rot).abs() > 0.2                                                      # where the shear is well conditioned
    inside_and_spread(shear[ok].float(), -22.5, 22.5)


def test_recipes_of_the_three_tasks():
    from ssl4gie_amd.data import FinetuneAugment
    from ssl4gie_amd.ops import IMAGENET_MEAN, IMAGENET_STD
    d = FinetuneAugment.depth(generator=_gen(2))
    factors, order, flags, sigma, flip, matrix = d.draw(512, CPU)
    assert d.blur_sigma is None and d.affine is None and not bool(sigma.any())
    assert matrix.tolist() == [IDENTITY] * 512                                           # depth: flips alone
    assert sorted(set(flip.tolist())) == [0, 1, 2, 3] and all(sorted(r) == [0, 1, 2, 3] for r in order.tolist())
    c = FinetuneAugment.classification(generator=_gen(3))
    assert c.fill == tuple((0.0 - m) / s for m, s in zip(IMAGENET_MEAN, IMAGENET_STD)) and c.blur_sigma == (0.001, 2.0)
    factors, order, flags, sigma, flip, matrix = c.draw(512, CPU)
    m = matrix.double()
    assert not bool(m[:, [2, 5]].any())                                                  # no translation
    assert float((m[:, 0] - m[:, 4]).abs().max()) < 1e-6 and float((m[:, 1] + m[:, 3]).abs().max()) < 1e-6
    assert float((m[:, 0] ** 2 + m[:, 1] ** 2 - 1.0).abs().max()) < 1e-6                 # a pure rotation
    ang = torch.rad2deg(torch.atan2(-m[:, 3], m[:, 4]))
    assert float(ang.min()) < -170 and float(ang.max()) > 170 and bool((sigma > 0).all())
    s = FinetuneAugment.segmentation()
    assert s.affine == dict(angle=180.0, translate=1.0 / 8.0, scale=(0.5, 1.5), shear=22.5) and s.size == 224
    assert s.color.jitter == (0.4, 0.5, 0.25, 0.01) and s.hflip and s.vflip and s.blur_sigma == (0.001, 2.0)
    none = FinetuneAugment(hflip=False, vflip=False, generator=_gen(4))
    assert not bool(none.draw(64, CPU)[4].any())
    for kw in (dict(size=12), dict(size=18), dict(blur_sigma=(0.0, 2.0)), dict(blur_sigma=(2.0, 1.0)),
               dict(affine=dict(rotate=3)), dict(fill="white")):
        with pytest.raises(ValueError):
            FinetuneAugment(**kw)
    FinetuneAugment(blur_sigma=(0.5, 4.0))                                               # 25 taps truncate any sigma, as torchvision's do


def test_bank_targets_and_no_cpu_fallback():
    from ssl4gie_amd import ops
    from ssl4gie_amd.data import DeviceImageBank, DeviceLoader, FinetuneAugment, RandomResizedCropFlip
    imgs = torch.zeros(4, 16, 16, 3, dtype=torch.uint8)
    assert DeviceImageBank(imgs).targets is None
    for dtype in (torch.uint8, torch.uint16, torch.int16, torch.float32):
        tgt = torch.zeros(4, 16, 16, dtype=dtype)
        assert DeviceImageBank(imgs, targets=tgt).targets is tgt
    for bad in (torch.zeros(4, 16, 16, dtype=torch.int64), torch.zeros(4, 16, 12, dtype=torch.uint8),
                torch.zeros(3, 16, 16, dtype=torch.uint8), torch.zeros(4, 16, 32, dtype=torch.uint8)[:, :, ::2], np.zeros((4, 16, 16), np.uint8)):
        with pytest.raises(ValueError):
            DeviceImageBank(imgs, targets=bad)
    bank = DeviceImageBank.from_uint8(imgs.numpy(), CPU, targets=np.zeros((4, 16, 16), np.uint16))
    assert bank.targets.dtype == torch.uint16 and len(bank) == 4 and bank[3] == (3, 0)
    t = FinetuneAugment.segmentation(16, generator=_gen(0))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        t(bank, torch.zeros(2, dtype=torch.int64))
    with pytest.raises(ValueError, match="stored at 32 x 32"):
        FinetuneAugment.segmentation(32)(bank, torch.zeros(2, dtype=torch.int64))
    x = torch.rand(2, 3, 16, 16)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.color_augment_ft(x, *t.draw(2, CPU)[:4])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.paired_warp(x, None, None, (0.0, 0.0, 0.0))
    # a bank with targets needs a transform that returns the pair
    loader = DeviceLoader(bank, 2, sampler=torch.utils.data.SequentialSampler(bank), transform=lambda bank, index: index)
    with pytest.raises(TypeError, match="targets"):
        next(iter(loader))
    loader = DeviceLoader(bank, 2, sampler=torch.utils.data.SequentialSampler(bank), transform=lambda bank, index: (index, index + 1))
    assert [tuple(a.tolist() for a in pair) for pair in loader] == [([0, 1], [1, 2]), ([2, 3], [3, 4])]


def test_pack_images_tool_packs_targets(tmp_path):
    from PIL import Image
    from ssl4gie_amd.data import DeviceImageBank
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import pack_images
    rng = np.random.default_rng(0)
    for d in ("images", "masks", "depth"):
        os.makedirs(tmp_path / d)
    masks, depths = [], []
    for k in range(3):
        Image.fromarray(rng.integers(0, 256, (20, 24, 3), dtype=np.uint8)).save(tmp_path / "images" / f"{k}.png")
        masks.append(rng.integers(0, 2, (20, 24), dtype=np.uint8) * 255)
        Image.fromarray(masks[-1]).convert("RGB").save(tmp_path / "masks" / f"{k}.png")     # masks come as RGB files
        depths.append(rng.integers(0, 65536, (16, 16)).astype(np.uint16))
        Image.fromarray(depths[-1]).save(tmp_path / "depth" / f"{k}.png")                   # mode I;16
    out = str(tmp_path / "b")
    assert pack_images.pack(str(tmp_path / "images"), out, 16, 16) == 3
    assert pack_images.pack_targets(str(tmp_path / "masks"), out, 16, 16, 3) == np.uint8
    got = np.load(out + ".targets.npy")
    assert got.dtype == np.uint8 and got.shape == (3, 16, 16)
    want = np.stack([np.asarray(Image.fromarray(m).convert("RGB").resize((16, 16)).convert("L")) for m in masks])
    assert np.array_equal(got, want)                                                       # PIL's default filter
    bank = DeviceImageBank.from_npy(out + ".npy", CPU, targets=out + ".targets.npy")
    assert bank.targets.dtype == torch.uint8 and np.array_equal(bank.targets.numpy(), want)
    assert pack_images.pack_targets(str(tmp_path / "depth"), out, 16, 16, 3) == np.uint16
    got = np.load(out + ".targets.npy")
    assert got.dtype == np.uint16 and np.array_equal(got, np.stack(depths))                # already 16 x 16: as stored
    bank = DeviceImageBank.from_npy(out + ".npy", CPU, targets=out + ".targets.npy", chunk_bytes=700)
    assert bank.targets.dtype == torch.uint16 and np.array_equal(bank.targets.numpy(), np.stack(depths))
    with pytest.raises(SystemExit):
        pack_images.pack_targets(str(tmp_path / "depth"), out, 16, 16, 4)                  # one target per image
    with pytest.raises(ValueError):
        DeviceImageBank.from_npy(out + ".npy", CPU, targets=out + ".labels.npy")


def test_multiplying_by_the_fp32_reciprocal_is_not_the_division():
    """why FinetuneAugment's [0, 1] images come from normalize_u8 and are called that, not `u8 / 255`: both it and
    view_sample_u8 multiply by fp32 1 / 255 (the statement of their rule, (v / 255 - mean) / std, folded into one
    multiply-add), which for 126 of the 256 levels is the neighbouring fp32 number of v / 255.  The targets of
    ssl4gie_paired_warp are true divisions."""
    v = torch.arange(256, dtype=torch.float32)
    folded = v * (torch.tensor(1.0) / torch.tensor(255.0))
    assert int((folded != v / 255.0).sum()) == 126
    assert float((folded.double() - v.double() / 255.0).abs().max()) < 2.0 ** -23     # never more than the neighbour


def test_header_declares_and_lib_binds_the_finetune_stage():
    from ssl4gie_amd import _lib
    txt = open(os.path.join(ROOT, "include", "ssl4gie_hip.h")).read()
    assert "ssl4gie_color_augment_ft / ssl4gie_paired_warp, joined revision 12" in txt
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    declared = set(re.findall(r"\b(ssl4gie_[a-z0-9_]+)\s*\(", txt))
    for name in ("ssl4gie_color_augment_ft", "ssl4gie_paired_warp"):
        assert name in declared and name in _lib.PROTOTYPES
    for name, value in (("SSL4GIE_TGT_U8", _lib.TGT_U8), ("SSL4GIE_TGT_U16", _lib.TGT_U16), ("SSL4GIE_TGT_F32", _lib.TGT_F32)):
        assert re.search(rf"#define {name} {value}\b", txt)
    assert _lib.ABI_VERSION == 13 and _lib.load().ssl4gie_abi_version() == 13


def test_finetune_entry_points_refuse_host_checkable_arguments_before_any_launch():
    """SSL4GIE_EARG with pointers that are never dereferenced (no GPU needed)"""
    from ssl4gie_amd import _lib
    L = _lib.load()
    m, s, z = (C.c_float * 3)(0, 0, 0), (C.c_float * 3)(1, 1, 1), (C.c_float * 3)(1, 0, 1)
    p, q, r = 4096, 1 << 20, 1 << 24  # non-null, 16-byte aligned, far apart
    need = L.ssl4gie_color_augment_workspace_bytes(2, 32)
    good = dict(x=p, out=q, B=2, S=32, factors=p, order=p, flags=p, sigma=p, mean=m, std=s, ws=p, ws_bytes=need)

    def color(**kw):
        a = {**good, **kw}
        return L.ssl4gie_color_augment_ft(a["x"], a["out"], a["B"], a["S"], a["factors"], a["order"], a["flags"],
                                          a["sigma"], a["mean"], a["std"], a["ws"], a["ws_bytes"], None)

    for name in ("x", "out", "factors", "order", "flags", "sigma", "mean", "std", "ws"):
        assert color(**{name: None}) == 1000, name
    assert color(S=12) == 1000 and color(S=18) == 1000 and color(S=8) == 1000        # reflect needs S > 12; S % 4
    assert color(B=0) == 1000 and color(std=z) == 1000 and color(out=p) == 1000       # ..., in place
    assert color(ws_bytes=need - 1) == 1000

    fill = (C.c_float * 3)(-1, -1, -1)
    base = dict(img=p, out=q, bank=r, dtype=_lib.TGT_U8, n=5, index=p, tgt_out=r + (1 << 20), matrix=p, flip=p, fill=fill,
                B=2, S=32)

    def warp(**kw):
        a = {**base, **kw}
        return L.ssl4gie_paired_warp(a["img"], a["out"], a["bank"], a["dtype"], a["n"], a["index"], a["tgt_out"],
                                     a["matrix"], a["flip"], a["fill"], 0.0, a["B"], a["S"], None)

    assert warp(img=None) == 1000 and warp(out=None) == 1000 and warp(fill=None) == 1000
    assert warp(out=p) == 1000                                                         # aliasing
    assert warp(out=p + 2 * 3 * 32 * 32 * 4 - 16) == 1000                              # overlapping, not identical
    assert warp(dtype=3) == 1000 and warp(dtype=-1) == 1000                            # a bad tgt_dtype
    assert warp(bank=None) == 1000                                                     # tgt_out without tgt_bank
    assert warp(tgt_out=None) == 1000 and warp(index=None) == 1000 and warp(n=0) == 1000
    assert warp(S=18) == 1000 and warp(S=0) == 1000 and warp(B=-1) == 1000
    assert warp(out=q + 4) == 1000                                                     # not 16-byte aligned
    # B = 0 is an empty batch, with or without a target, a matrix or flips: accepted, nothing launched
    assert warp(B=0) == 0
    assert warp(B=0, bank=None, index=None, tgt_out=None, matrix=None, flip=None) == 0
