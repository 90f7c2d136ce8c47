"""CPU: the host side of the MAE fine-tuning recipe (reference Models/mae/main_finetune.py): the classifier's
state_dict schema and checkpoint path, layer-wise learning-rate decay groups, position-table interpolation, the
Mixup tables as a pure function of a RandomState, and the torch formulations of Mixup and the two losses against the
fp64 restatements of tests/finetune_checks.py."""
import argparse
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import finetune_checks as fc
from conftest import ROOT, rel_err


@pytest.fixture(scope="module")
def vitb():
    from ssl4gie_amd.Models.mae import models_vit
    torch.manual_seed(0)
    return models_vit.vit_base_patch16(global_pool=True, num_classes=1000, drop_path_rate=0.1)


def test_classifier_schema_global_pool(vitb):
    sd = vitb.state_dict()
    assert len(sd) == 152
    assert "fc_norm.weight" in sd and "fc_norm.bias" in sd and not any(k.startswith("norm.") for k in sd)
    assert vitb.pos_embed.requires_grad and tuple(vitb.pos_embed.shape) == (1, 197, 768)
    assert {"cls_token", "pos_embed", "patch_embed.proj.weight", "patch_embed.proj.bias", "blocks.11.mlp.fc2.bias",
            "head.weight", "head.bias"} <= set(sd)
    assert vitb.no_weight_decay() == {"pos_embed", "cls_token"}
    # stochastic depth: linspace(0, rate, depth), a plain float per block, no parameter and no buffer
    rates = [b.drop_path for b in vitb.blocks]
    assert all(isinstance(r, float) for r in rates)
    assert np.allclose(rates, fc.linspace_rates(0.1, 12), atol=1e-7) and rates[0] == 0.0
    assert not any("drop" in k for k in sd) and not list(vitb.buffers())


def test_classifier_schema_cls_token():
    from ssl4gie_amd.Models.mae import models_vit
    m = models_vit.vit_base_patch16(global_pool=False, num_classes=10)
    sd = m.state_dict()
    assert "norm.weight" in sd and "norm.bias" in sd and not any(k.startswith("fc_norm") for k in sd)
    assert len(sd) == 152 and tuple(sd["head.weight"].shape) == (10, 768)
    assert all(b.drop_path == 0.0 for b in m.blocks)


def test_block_keeps_its_state_dict_with_a_drop_rate():
    from ssl4gie_amd.Models.vit_layers import Block
    a, b = Block(64, 2), Block(64, 2, drop_path=0.3)
    assert list(a.state_dict()) == list(b.state_dict()) and a.drop_path == 0.0 and b.drop_path == 0.3


def test_mae_checkpoint_loads_as_main_finetune_expects(vitb):
    from ssl4gie_amd.Models.mae import models_mae
    from ssl4gie_amd.Models.mae.util.pos_embed import interpolate_pos_embed
    torch.manual_seed(1)
    mae = models_mae.mae_vit_base_patch16()
    ck = {k: v.clone() for k, v in mae.state_dict().items()}
    interpolate_pos_embed(vitb, ck)   # same grid: the table is left alone
    assert torch.equal(ck["pos_embed"], mae.state_dict()["pos_embed"])
    msg = vitb.load_state_dict(ck, strict=False)
    assert set(msg.missing_keys) == {"head.weight", "head.bias", "fc_norm.weight", "fc_norm.bias"}
    unexpected = set(msg.unexpected_keys)
    assert {"mask_token", "norm.weight", "norm.bias", "decoder_pos_embed"} <= unexpected
    assert all(k in ("mask_token", "norm.weight", "norm.bias") or k.startswith("decoder_") for k in unexpected)
    own = vitb.state_dict()
    shared = [k for k in ck if k in own]
    assert len(shared) == 148 and all(torch.equal(own[k], ck[k]) for k in shared)


def test_huge_patch14_is_refused():
    from ssl4gie_amd.Models.mae import models_vit
    with pytest.raises(NotImplementedError):
        models_vit.vit_huge_patch14(global_pool=True)
    assert models_vit.vit_large_patch16(num_classes=3, global_pool=True).blocks[23].attn.qkv.weight.shape == (3072, 1024)


def test_param_groups_lrd(vitb):
    from ssl4gie_amd.Models.mae.util import lr_sched
    from ssl4gie_amd.Models.mae.util.lr_decay import get_layer_id_for_vit, param_groups_lrd
    groups = param_groups_lrd(vitb, 0.05, no_weight_decay_list=vitb.no_weight_decay(), layer_decay=0.75)
    assert len(groups) == 28
    names = {id(p): n for n, p in vitb.named_parameters()}
    seen = {}
    for gi, g in enumerate(groups):
        assert set(g) == {"lr_scale", "weight_decay", "params"}
        layers = {fc.layer_of(names[id(p)], 12) for p in g["params"]}
        assert len(layers) == 1
        layer = layers.pop()
        assert g["lr_scale"] == pytest.approx(0.75 ** (13 - layer), rel=1e-12)
        assert g["weight_decay"] in (0.0, 0.05)
        for p in g["params"]:
            n = names[id(p)]
            assert n not in seen, n
            seen[n] = (layer, g["weight_decay"])
            assert get_layer_id_for_vit(n, 13) == layer
            no_decay = p.ndim == 1 or n in ("pos_embed", "cls_token")
            assert g["weight_decay"] == (0.0 if no_decay else 0.05), n
    assert set(seen) == {n for n, p in vitb.named_parameters() if p.requires_grad}   # every one, exactly once
    for n in ("cls_token", "pos_embed", "patch_embed.proj.bias"):
        assert seen[n] == (0, 0.0)
    assert seen["patch_embed.proj.weight"] == (0, 0.05)
    assert seen["head.weight"] == (13, 0.05)
    for n in ("fc_norm.weight", "fc_norm.bias", "head.bias"):
        assert seen[n] == (13, 0.0)
    assert seen["blocks.4.attn.qkv.weight"] == (5, 0.05) and seen["blocks.4.norm1.weight"] == (5, 0.0)
    # the schedule scales every group by its lr_scale
    opt = argparse.Namespace(param_groups=[dict(g) for g in groups])
    args = argparse.Namespace(lr=1e-3, min_lr=1e-6, warmup_epochs=5, epochs=50)
    for epoch in (2.5, 20.0):
        lr = lr_sched.adjust_learning_rate(opt, epoch, args)
        assert all(g["lr"] == lr * g["lr_scale"] for g in opt.param_groups)
    # a frozen parameter stays out
    vitb.cls_token.requires_grad_(False)
    try:
        g2 = param_groups_lrd(vitb, 0.05, vitb.no_weight_decay(), 0.75)
        assert sum(len(g["params"]) for g in g2) == 151
    finally:
        vitb.cls_token.requires_grad_(True)


def test_interpolate_pos_embed_bicubic():
    from ssl4gie_amd.Models.mae import models_vit
    from ssl4gie_amd.Models.mae.util.pos_embed import interpolate_pos_embed
    m = models_vit.VisionTransformer(img_size=384, embed_dim=64, depth=1, num_heads=2, num_classes=4)   # 24 x 24 grid
    g = torch.Generator().manual_seed(7)
    table = torch.randn(1, 197, 64, generator=g)
    ck = {"pos_embed": table.clone()}
    interpolate_pos_embed(m, ck)
    got = ck["pos_embed"]
    assert tuple(got.shape) == (1, 1 + 24 * 24, 64) == tuple(m.pos_embed.shape)
    assert torch.equal(got[:, :1], table[:, :1])   # the cls row is kept
    want = F.interpolate(table[:, 1:].reshape(1, 14, 14, 64).permute(0, 3, 1, 2), size=(24, 24), mode="bicubic",
                         align_corners=False).permute(0, 2, 3, 1).reshape(1, 576, 64)
    assert torch.equal(got[:, 1:], want)
    m.load_state_dict(ck, strict=False)
    ck2 = {"other": torch.zeros(1)}
    interpolate_pos_embed(m, ck2)
    assert set(ck2) == {"other"}


MIX_KW = [dict(mixup_alpha=0.8, cutmix_alpha=1.0), dict(mixup_alpha=0.0, cutmix_alpha=1.0),
          dict(mixup_alpha=0.8, cutmix_alpha=0.0), dict(mixup_alpha=0.8, cutmix_alpha=1.0, cutmix_minmax=(0.2, 0.8)),
          dict(mixup_alpha=0.8, cutmix_alpha=1.0, prob=0.5)]


@pytest.mark.parametrize("mode", ["batch", "pair", "elem"])
@pytest.mark.parametrize("B", [6, 5])
def test_mixup_tables(mode, B):
    from ssl4gie_amd.data import mixup_tables
    H, W = 32, 30
    for ki, kw in enumerate(MIX_KW):
        for seed in range(6):
            lam, box, use = mixup_tables(np.random.RandomState(100 * ki + seed), B, H, W, mode=mode, **kw)
            lam2, box2, use2 = mixup_tables(np.random.RandomState(100 * ki + seed), B, H, W, mode=mode, **kw)
            assert np.array_equal(lam, lam2) and np.array_equal(box, box2) and np.array_equal(use, use2)   # pure
            assert lam.dtype == np.float32 and box.dtype == np.int32 and use.dtype == np.uint8
            assert lam.shape == (B,) and box.shape == (B, 4) and use.shape == (B,)
            assert np.all((lam >= 0) & (lam <= 1))
            y0, y1, x0, x1 = box.T
            assert np.all((0 <= y0) & (y0 <= y1) & (y1 <= H) & (0 <= x0) & (x0 <= x1) & (x1 <= W))
            area = (y1 - y0).astype(np.float64) * (x1 - x0)
            cut = use != 0
            assert np.array_equal(lam[cut], (1.0 - area[cut] / float(H * W)).astype(np.float32))   # corrected lambda
            assert np.all(use[lam == 1.0] == 1) and np.all(area[lam == 1.0] == 0)   # unmixed: the empty box
            if kw.get("cutmix_alpha") == 0.0:
                assert np.all(area == 0)
            if mode == "batch":
                assert np.all(lam == lam[0]) and np.all(box == box[0]) and np.all(use == use[0])
            if mode == "pair":
                assert np.array_equal(lam, lam[::-1]) and np.array_equal(box, box[::-1]) and np.array_equal(use, use[::-1])
                if B % 2:
                    assert lam[B // 2] == 1.0
    lam, box, use = mixup_tables(np.random.RandomState(0), B, H, W, mode=mode, mixup_alpha=0.8, cutmix_alpha=1.0, prob=0.0)
    assert np.all(lam == 1.0) and np.all(box == 0)
    if mode == "elem":   # per-sample draws do differ
        lam, _, _ = mixup_tables(np.random.RandomState(1), 6, H, W, mode=mode, mixup_alpha=0.8)
        assert len(set(lam.tolist())) == 6
    with pytest.raises(ValueError):
        mixup_tables(np.random.RandomState(0), B, H, W, mode="rows")
    with pytest.raises(ValueError):
        mixup_tables(np.random.RandomState(0), B, H, W, mixup_alpha=0.0, cutmix_alpha=0.0)


@pytest.mark.parametrize("mode", ["batch", "pair", "elem"])
@pytest.mark.parametrize("B", [6, 5])
def test_mixup_torch_formulation_on_cpu_tensors(mode, B):
    from ssl4gie_amd.data import Mixup
    g = torch.Generator().manual_seed(11)
    C = 7
    for seed in range(4):
        x = torch.randn(B, 3, 16, 12, generator=g)
        y = torch.randint(0, C, (B,), generator=g)
        mix = Mixup(mixup_alpha=0.8, cutmix_alpha=1.0, mode=mode, label_smoothing=0.1, num_classes=C,
                    rng=np.random.RandomState(seed))
        lam, box, use = Mixup(mixup_alpha=0.8, cutmix_alpha=1.0, mode=mode, label_smoothing=0.1, num_classes=C,
                              rng=np.random.RandomState(seed)).draw(B, 16, 12)
        x0 = x.clone()
        xm, soft = mix(x, y)
        assert xm is x and soft.dtype == torch.float32 and tuple(soft.shape) == (B, C)   # in place, as timm
        want = fc.mixup_images(x0.double(), torch.from_numpy(lam), torch.from_numpy(box), torch.from_numpy(use))
        assert rel_err(xm, want) < 1e-6
        # ... and bit for bit against the same statement in fp32
        assert torch.equal(xm, fc.mixup_images(x0, torch.from_numpy(lam), torch.from_numpy(box), torch.from_numpy(use)))
        st = fc.mixup_targets(y, torch.from_numpy(lam), C, 0.1)
        assert rel_err(soft, st) < 1e-6 and float((soft.sum(1) - 1).abs().max()) < 1e-6


@pytest.mark.parametrize("B,C", [(1, 1), (5, 6), (5, 1000), (3, 1003)])
def test_loss_torch_formulations_on_cpu_tensors(B, C):
    from ssl4gie_amd.losses import LabelSmoothingCrossEntropy, SoftTargetCrossEntropy
    g = torch.Generator().manual_seed(B * 1000 + C)
    x = torch.randn(B, C, generator=g) * 3
    t = torch.rand(B, C, generator=g)
    t = t / t.sum(1, keepdim=True)
    y = torch.randint(0, C, (B,), generator=g)
    for mod, args, ref in ((SoftTargetCrossEntropy(), (t,), fc.soft_target_ce),
                           (LabelSmoothingCrossEntropy(0.1), (y,), lambda a, b: fc.label_smoothing_ce(a, b, 0.1))):
        l64, d64 = fc.loss_and_grad(ref, x, *args)
        xr = x.clone().requires_grad_(True)
        loss = mod(xr, *args)
        loss.backward()
        assert abs(float(loss.detach()) - float(l64)) <= 1e-5 * max(1.0, abs(float(l64)))
        assert rel_err(xr.grad, d64) < 1e-5 or float(d64.abs().max()) < 1e-12


def test_new_entry_points_are_declared_bound_and_exported():
    import ctypes
    from ssl4gie_amd import _lib
    txt = open(os.path.join(ROOT, "include", "ssl4gie_hip.h")).read()
    declared = set(re.findall(r"\b(ssl4gie_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", txt, flags=re.S)))
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("ssl4gie_block_dp_workspace_bytes", "ssl4gie_block_fwd_dp", "ssl4gie_block_bwd_dp",
                 "ssl4gie_drop_path_add", "ssl4gie_drop_path_scale_cast", "ssl4gie_mixup", "ssl4gie_mixup_target",
                 "ssl4gie_soft_cross_entropy_workspace_bytes", "ssl4gie_soft_cross_entropy"):
        assert name in declared and name in _lib.PROTOTYPES and hasattr(lib, name), name
    L = _lib.load()
    assert _lib.ABI_VERSION == 13 and L.ssl4gie_abi_version() == 13
    # the stochastic-depth slots belong to their own query: the plain one keeps its value
    for dt, es in ((_lib.BF16, 2), (_lib.F32, 4)):
        d = _lib.BlockDims(5, 197, 768, 12, 3072, dt, 1e-6)
        plain, dp = L.ssl4gie_block_workspace_bytes(ctypes.byref(d)), L.ssl4gie_block_dp_workspace_bytes(ctypes.byref(d))
        T = 5 * 197
        assert dp == plain + T * 768 * 4 + 2 * T * 768 * es   # (all three slots are multiples of 256 bytes here)
    assert L.ssl4gie_soft_cross_entropy_workspace_bytes(5, 1000) > 0
