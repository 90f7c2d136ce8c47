"""CPU: the conv-stem ViT zoo (ssl4gie_amd/Models/moco_v3/vits.py) against what the reference's own classes report
(tests/golden/g19_convstem.npz, `zoo/`): same state_dict keys and shapes, same parameter counts, depth 11, the same
frozen-parameter pattern with and without stop_grad_conv1, and the reference's constructor contract of ConvStem."""
import numpy as np
import pytest
import torch.nn as nn

from conftest import load_golden


@pytest.mark.parametrize("name,embed,params", [("vit_conv_small", 384, 20715952), ("vit_conv_base", 768, 82396768)])
def test_conv_stem_zoo_matches_the_reference(name, embed, params):
    from ssl4gie_amd.Models.moco_v3 import vits
    g = load_golden("g19_convstem.npz")
    assert name in vits.__all__ and sorted(vits.__all__) == ["vit_base", "vit_conv_base", "vit_conv_small", "vit_small"]
    m = getattr(vits, name)(num_classes=256)
    sd = m.state_dict()
    keys = sorted(sd)
    assert keys == g[f"zoo/{name}/keys"].tolist()
    assert [",".join(str(d) for d in sd[k].shape) for k in keys] == g[f"zoo/{name}/shapes"].tolist()
    assert sum(p.numel() for p in m.parameters()) == int(g[f"zoo/{name}/params"]) == params
    assert len(m.blocks) == int(g[f"zoo/{name}/depth"]) == 11
    assert m.embed_dim == embed and m.num_heads == 12
    stem = [k for k in keys if k.startswith("patch_embed.")]
    assert len(stem) == 26
    for stop in (False, True):
        mm = getattr(vits, name)(num_classes=256, stop_grad_conv1=stop)
        frozen = sorted(k for k, p in mm.named_parameters() if not p.requires_grad)
        assert frozen == g[f"zoo/{name}/{'stop' if stop else 'plain'}/frozen"].tolist() == ["pos_embed"]


def test_conv_stem_constructor_contract():
    from ssl4gie_amd.Models.moco_v3.vits import ConvStem
    s = ConvStem(img_size=224, patch_size=16, in_chans=3, embed_dim=384, norm_layer=None, flatten=True)
    assert (s.img_size, s.patch_size, s.grid_size, s.num_patches, s.flatten) == ((224, 224), (16, 16), (14, 14), 196, True)
    assert isinstance(s.norm, nn.Identity) and isinstance(s.proj, nn.Sequential) and len(s.proj) == 13
    widths = [48, 96, 192, 384]
    for i, c in enumerate(widths):
        conv, bn, act = s.proj[3 * i], s.proj[3 * i + 1], s.proj[3 * i + 2]
        assert isinstance(conv, nn.Conv2d) and conv.bias is None and conv.kernel_size == (3, 3) and conv.stride == (2, 2)
        assert conv.weight.shape == (c, 3 if i == 0 else widths[i - 1], 3, 3)
        assert isinstance(bn, nn.BatchNorm2d) and bn.num_features == c and isinstance(act, nn.ReLU)
    assert s.proj[12].weight.shape == (384, 384, 1, 1) and s.proj[12].bias is not None
    assert isinstance(ConvStem(embed_dim=64, norm_layer=nn.LayerNorm).norm, nn.LayerNorm)
    with pytest.raises(AssertionError):
        ConvStem(patch_size=8)
    with pytest.raises(AssertionError):
        ConvStem(embed_dim=100)


def test_patch_embed_models_are_untouched_by_the_conv_stem():
    """stop_grad_conv1 still freezes the 16 x 16 patch projection of vit_small / vit_base, and only that"""
    from ssl4gie_amd.Models.moco_v3 import vits
    m = vits.vit_small(num_classes=16, stop_grad_conv1=True)
    frozen = sorted(k for k, p in m.named_parameters() if not p.requires_grad)
    assert frozen == ["patch_embed.proj.bias", "patch_embed.proj.weight", "pos_embed"]
    assert len(m.blocks) == 12
