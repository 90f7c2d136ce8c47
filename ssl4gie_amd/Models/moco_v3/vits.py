"""MoCo-v3 ViT variants on the engine (reference `Models/moco_v3/vits.py:25-143`): a timm
VisionTransformer with a FIXED 2-D sin-cos position embedding (cls row zero), MoCo's init (uniform
qkv per third, xavier elsewhere, zero biases, cls ~ N(0, 1e-6)), optional stop-gradient on the patch
embedding, and a `head` Linear that MoCo_ViT replaces by its projector.  `vit_base(**kw)` is the
factory `main_moco.py:181-183` calls through `partial(vits.__dict__[arch], stop_grad_conv1=...)`.

`vit_conv_small` / `vit_conv_base` replace the 16 x 16 patch projection by `ConvStem` (four 3x3 stride-2
convolution + BatchNorm + ReLU stages and a 1x1 projection; Xiao et al., "Early Convolutions Help Transformers
See Better") and drop one of the twelve blocks.  The stem runs on the engine through
`_ViTBackbone._conv_stem_tokens`.
"""
from __future__ import annotations

import math

import torch
import torch.nn as nn

from ..models import _ViTBackbone, moco_sincos_pos_embed
from ..vit_layers import PatchEmbed, _pair

__all__ = [
    'vit_small',
    'vit_base',
    'vit_conv_small',
    'vit_conv_base',
]


class ConvStem(nn.Module):
    """Parameter and buffer holder of the reference's ConvStem (`vits.py:72-112`), same constructor, attributes and
    state_dict keys: `proj` is the Sequential of 13 children (Conv2d 3x3 s2 without bias, BatchNorm2d, ReLU) x 4 at
    widths embed_dim / 8, / 4, / 2, / 1, then Conv2d 1x1 with bias.  The children hold no arithmetic."""

    def __init__(self, img_size=224, patch_size=16, in_chans=3, embed_dim=768, norm_layer=None, flatten=True):
        super().__init__()
        assert patch_size == 16, 'ConvStem only supports patch size of 16'
        assert embed_dim % 8 == 0, 'Embed dimension must be divisible by 8 for ConvStem'
        self.img_size = _pair(img_size)
        self.patch_size = _pair(patch_size)
        self.grid_size = (self.img_size[0] // self.patch_size[0], self.img_size[1] // self.patch_size[1])
        self.num_patches = self.grid_size[0] * self.grid_size[1]
        self.flatten = flatten
        layers, cin = [], 3   # (the reference's stem starts from 3 channels whatever in_chans says)
        for k in (8, 4, 2, 1):
            cout = embed_dim // k
            layers += [nn.Conv2d(cin, cout, kernel_size=3, stride=2, padding=1, bias=False),
                       nn.BatchNorm2d(cout), nn.ReLU(inplace=True)]
            cin = cout
        layers.append(nn.Conv2d(cin, embed_dim, kernel_size=1))
        self.proj = nn.Sequential(*layers)
        self.norm = norm_layer(embed_dim) if norm_layer else nn.Identity()


class VisionTransformerMoCo(_ViTBackbone):
    def __init__(self, embed_dim=768, depth=12, num_heads=12, num_classes=1000, stop_grad_conv1=False,
                 embed_layer=None, **kwargs):
        super().__init__()
        self._build_trunk(embed_dim, depth, num_heads, embed_layer=embed_layer)
        self.head = nn.Linear(embed_dim, num_classes)
        self.pos_embed.requires_grad = False
        with torch.no_grad():
            self.pos_embed.copy_(moco_sincos_pos_embed(embed_dim, self.patch_embed.grid_size))
            for name, m in self.named_modules():
                if isinstance(m, nn.Linear):
                    if "qkv" in name:  # treat the weights of Q, K, V separately
                        val = math.sqrt(6. / float(m.weight.shape[0] // 3 + m.weight.shape[1]))
                        nn.init.uniform_(m.weight, -val, val)
                    else:
                        nn.init.xavier_uniform_(m.weight)
                    nn.init.zeros_(m.bias)
            nn.init.normal_(self.cls_token, std=1e-6)
            if isinstance(self.patch_embed, PatchEmbed):
                ps = self.patch_embed.patch_size
                val = math.sqrt(6. / float(3 * ps[0] * ps[1] + embed_dim))
                nn.init.uniform_(self.patch_embed.proj.weight, -val, val)
                nn.init.zeros_(self.patch_embed.proj.bias)
        # (a ConvStem keeps PyTorch's default Conv2d / BatchNorm2d init and is never frozen: reference :43-51)
        if stop_grad_conv1 and isinstance(self.patch_embed, PatchEmbed):
            self.patch_embed.proj.weight.requires_grad = False
            self.patch_embed.proj.bias.requires_grad = False
        self.dense, self.det, self.frozen, self.out_token, self.head_flag = None, False, False, "cls", False

    def forward_cls(self, imgs):
        """final-norm cls token, fp32 [B, D] (timm global_pool='token')"""
        return self._trunk(imgs, None)[:, 0]

    def forward(self, imgs):
        from ...engine import LinearFn
        x = self.forward_cls(imgs)
        return LinearFn.apply(x.to(self.dtype_).contiguous(), self.head.weight, self.head.bias,
                              self.dtype_, torch.float32, self.sink(), self.lp_cache)


def vit_small(**kwargs):
    return VisionTransformerMoCo(embed_dim=384, depth=12, num_heads=12, **kwargs)


def vit_base(**kwargs):
    return VisionTransformerMoCo(embed_dim=768, depth=12, num_heads=12, **kwargs)


def vit_conv_small(**kwargs):
    return VisionTransformerMoCo(embed_dim=384, depth=11, num_heads=12, embed_layer=ConvStem, **kwargs)  # minus one block


def vit_conv_base(**kwargs):
    return VisionTransformerMoCo(embed_dim=768, depth=11, num_heads=12, embed_layer=ConvStem, **kwargs)  # minus one block
