"""CPU: the host / torch-op side of the colour augmentation (ssl4gie_amd.data.ColorAugment, MoCoV3Views) — the
parameter draw against ColorJitter.get_params' distribution — and the C ABI declaration of ssl4gie_color_augment
with the arguments it refuses before any launch."""
import ctypes as C
import itertools
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT

CPU = torch.device("cpu")


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def test_draw_is_seeded_and_the_generator_advances():
    from ssl4gie_amd.data import ColorAugment
    t = ColorAugment(generator=_gen(5))
    a = t.draw(64, CPU)
    b = ColorAugment(generator=_gen(5)).draw(64, CPU)
    assert all(torch.equal(p, q) for p, q in zip(a, b))
    c = t.draw(64, CPU)
    assert not torch.equal(a[0], c[0]) and not torch.equal(a[3], c[3])
    factors, order, flags, sigma = a
    assert factors.dtype == torch.float32 and tuple(factors.shape) == (64, 4) and factors.is_contiguous()
    assert order.dtype == torch.uint8 and tuple(order.shape) == (64, 4) and order.is_contiguous()
    assert flags.dtype == torch.uint8 and tuple(flags.shape) == (64,)
    assert sigma.dtype == torch.float32 and tuple(sigma.shape) == (64,)


def test_draw_follows_get_params():
    from ssl4gie_amd.data import ColorAugment
    B = 4096
    t = ColorAugment(solarize_p=0.0, blur_p=1.0, generator=_gen(1))
    factors, order, flags, sigma = t.draw(B, CPU)
    rows = [tuple(r) for r in order.tolist()]
    skip = torch.tensor([r == (255,) * 4 for r in rows])
    perms = set(itertools.permutations(range(4)))
    assert all(r in perms or r == (255,) * 4 for r in rows)          # a permutation of 0..3, or all skipped
    assert {r for r in rows if r in perms} == perms                   # all 24 occur
    assert 0.15 < float(skip.float().mean()) < 0.25                   # jitter_p = 0.8
    ident = torch.tensor([1.0, 1.0, 1.0, 0.0])
    assert bool((factors[skip] == ident).all())                       # skip rows carry identity factors
    # factors inside their ranges (to the float32 rounding of the end points), and spread over them
    f32 = lambda v: torch.tensor(v, dtype=torch.float32)
    for k, (lo, hi) in enumerate(((0.6, 1.4), (0.6, 1.4), (0.8, 1.2), (-0.1, 0.1))):
        col = factors[~skip, k]
        assert bool((col >= f32(lo)).all()) and bool((col <= f32(hi)).all())
        assert float(col.min()) < lo + 0.02 * (hi - lo) and float(col.max()) > hi - 0.02 * (hi - lo)
        assert abs(float(col.double().mean()) - 0.5 * (lo + hi)) < 0.02 * (hi - lo)
    assert t.ranges() == [(0.6, 1.4), (0.6, 1.4), (0.8, 1.2), (-0.1, 0.1)]
    assert bool((sigma >= f32(0.1)).all()) and bool((sigma <= f32(2.0)).all())       # blur_p = 1: no sigma is 0
    assert bool((flags & 2 == 0).all()) and 0.15 < float((flags & 1).float().mean()) < 0.25
    # the second view's recipe: sigma in {0} u [0.1, 2], solarize bits set
    factors, order, flags, sigma = ColorAugment(blur_p=0.1, solarize_p=0.2, generator=_gen(2)).draw(B, CPU)
    on = sigma != 0
    assert 0.07 < float(on.float().mean()) < 0.13
    assert bool((sigma[on] >= f32(0.1)).all()) and bool((sigma[on] <= f32(2.0)).all())
    assert 0.16 < float(((flags & 2) != 0).float().mean()) < 0.24 and int(flags.max()) <= 3
    # brightness above 1 floors its range at 0; an op with value 0 is left out of the order, as torchvision does
    wide = ColorAugment(brightness=1.5, hue=0.0, jitter_p=1.0, generator=_gen(3))
    assert wide.ranges()[0] == (0.0, 2.5) and wide.ranges()[3] == (0.0, 0.0)
    factors, order, _, _ = wide.draw(512, CPU)
    assert bool((factors[:, 0] >= 0).all()) and bool((factors[:, 3] == 0).all())
    assert all(sorted(r) == [0, 1, 2, 255] for r in order.tolist())
    # jitter never applied, blur never applied
    factors, order, flags, sigma = ColorAugment(jitter_p=0.0, blur_p=0.0, gray_p=0.0, generator=_gen(4)).draw(64, CPU)
    assert bool((order == 255).all()) and bool((factors == ident).all()) and not bool(sigma.any()) and not bool(flags.any())


def test_constructor_refusals():
    from ssl4gie_amd.data import ColorAugment
    for kw in (dict(blur_sigma=(0.1, 2.5)), dict(blur_sigma=(-0.1, 2.0)), dict(blur_sigma=(1.5, 1.0)), dict(hue=0.6),
               dict(hue=-0.1), dict(brightness=-0.4), dict(contrast=-1.0), dict(saturation=-0.2), dict(jitter_p=1.5),
               dict(solarize_p=-0.1)):
        with pytest.raises(ValueError):
            ColorAugment(**kw)
    ColorAugment(hue=0.5, blur_sigma=(0.0, 2.0))


def test_no_cpu_fallback():
    from ssl4gie_amd import ops
    from ssl4gie_amd.data import ColorAugment, DeviceImageBank, MoCoV3Views
    x = torch.rand(2, 3, 8, 8)
    t = ColorAugment(generator=_gen(0))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        t(x)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.color_augment(x, *t.draw(2, CPU))
    bank = DeviceImageBank(torch.zeros(4, 12, 12, 3, dtype=torch.uint8))
    views = MoCoV3Views(8, generator=_gen(0))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        views(bank, torch.zeros(2, dtype=torch.int64))
    # the recipe of each view (main_moco.py:262-285)
    assert [c.blur_p for c in views.colors] == [1.0, 0.1] and [c.solarize_p for c in views.colors] == [0.0, 0.2]
    assert all(c.jitter == (0.4, 0.4, 0.2, 0.1) and c.jitter_p == 0.8 and c.gray_p == 0.2 for c in views.colors)
    assert all(c.interpolation == "bilinear" and c.scale == (0.08, 1.0) and c.mean == (0.0, 0.0, 0.0)
               and c.std == (1.0, 1.0, 1.0) and c.size == 8 for c in views.crops)


def test_header_declares_and_lib_binds_the_colour_stage():
    from ssl4gie_amd import _lib
    txt = open(os.path.join(ROOT, "include", "ssl4gie_hip.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    declared = set(re.findall(r"\b(ssl4gie_[a-z0-9_]+)\s*\(", txt))
    for name in ("ssl4gie_color_augment", "ssl4gie_color_augment_workspace_bytes"):
        assert name in declared and name in _lib.PROTOTYPES
    assert _lib.ABI_VERSION == 13 and _lib.load().ssl4gie_abi_version() == 13


def test_color_augment_refuses_host_checkable_arguments_before_any_launch():
    """SSL4GIE_EARG with pointers that are never dereferenced (no GPU needed)"""
    from ssl4gie_amd import _lib
    L = _lib.load()
    m, s, z = (C.c_float * 3)(0, 0, 0), (C.c_float * 3)(1, 1, 1), (C.c_float * 3)(1, 0, 1)
    p, q = 4096, 8192  # any two non-null values
    need = L.ssl4gie_color_augment_workspace_bytes(2, 32)
    assert need >= 2 * 4 and L.ssl4gie_color_augment_workspace_bytes(256, 224) >= 256 * 4
    assert L.ssl4gie_color_augment_workspace_bytes(0, 32) == 0 and L.ssl4gie_color_augment_workspace_bytes(2, 30) == 0
    good = dict(x=p, out=q, B=2, S=32, factors=p, order=p, flags=p, sigma=p, mean=m, std=s, ws=p, ws_bytes=need)

    def call(**kw):
        a = {**good, **kw}
        return L.ssl4gie_color_augment(a["x"], a["out"], a["B"], a["S"], a["factors"], a["order"], a["flags"], a["sigma"],
                                       a["mean"], a["std"], a["ws"], a["ws_bytes"], None)

    for name in ("x", "out", "factors", "order", "flags", "sigma", "mean", "std", "ws"):
        assert call(**{name: None}) == 1000, name                               # a null pointer
    assert call(B=0) == 1000 and call(B=-3) == 1000                             # B < 1
    assert call(S=4) == 1000 and call(S=0) == 1000 and call(S=30) == 1000       # S < 8, S % 4
    assert call(std=z) == 1000                                                  # a std entry equal to 0
    assert call(out=p) == 1000                                                  # in place
    assert call(ws_bytes=need - 1) == 1000 and call(ws_bytes=0) == 1000         # workspace too small
    assert call(B=3) == 1000                                                    # ... for this B
