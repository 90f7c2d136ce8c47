"""The classifier MAE fine-tunes (reference `Models/mae/models_vit.py:20-74`): timm's `VisionTransformer` with an
optional global average pool, on the MI355X engine.

State_dict keys are timm's: `cls_token`, `pos_embed` (trainable), `patch_embed.proj.*`, `blocks.i.*`, `head.*` and
`norm.*` — or, with `global_pool=True`, `fc_norm.*` and no `norm.*` (reference :27-32), so an MAE checkpoint loads
with `strict=False` exactly as `main_finetune.py:236-257` expects.  timm is not installed: the rules below (key
names, truncated-normal initialisation, `linspace` stochastic-depth schedule) are restated from its published source.

Forward (reference :34-53): patch embedding + [cls | tokens] + pos_embed, the block stack with stochastic depth
(engine.run_blocks draws timm's per-sample factors for the whole stack at once), then either the mean over the patch
tokens followed by `fc_norm`, or `norm` and the cls row; `head` gives fp32 logits.  `pos_drop` is the identity
(drop_rate is 0 in the recipe).

`head` is an nn.Linear, an nn.Identity, or the linear probe's `Sequential(BatchNorm1d(affine=False), Linear)`
(reference `main_linprobe.py:222`; state keys `head.0.running_mean`, `head.0.running_var`,
`head.0.num_batches_tracked`, `head.1.weight`, `head.1.bias`): the BatchNorm runs in the engine's BatchNorm kernels,
then the product.  Anything else raises TypeError.  `forward_head(feats)` drives the head on given features.
"""
from __future__ import annotations

from functools import partial

import torch
import torch.nn as nn

from ...engine import EngineModule, PatchEmbedFn
from ..vit_layers import Block, PatchEmbed


class VisionTransformer(EngineModule):
    """Vision Transformer with support for global average pooling (engine-backed)."""

    def __init__(self, global_pool=False, img_size=224, patch_size=16, in_chans=3, num_classes=1000,
                 embed_dim=768, depth=12, num_heads=12, mlp_ratio=4., qkv_bias=True, drop_path_rate=0.,
                 norm_layer=None):
        super().__init__()
        norm_layer = norm_layer or partial(nn.LayerNorm, eps=1e-6)
        self.num_classes = num_classes
        self.num_features = self.embed_dim = embed_dim
        self.num_heads = num_heads
        self.global_pool = global_pool
        self.patch_embed = PatchEmbed(img_size, patch_size, in_chans, embed_dim)
        n = self.patch_embed.num_patches
        self.cls_token = nn.Parameter(torch.zeros(1, 1, embed_dim))
        self.pos_embed = nn.Parameter(torch.zeros(1, n + 1, embed_dim))
        rates = torch.linspace(0, drop_path_rate, depth).tolist()  # stochastic depth decay rule
        self.blocks = nn.ModuleList([Block(embed_dim, num_heads, mlp_ratio, qkv_bias=qkv_bias, norm_layer=norm_layer,
                                           drop_path=rates[i]) for i in range(depth)])
        if global_pool:
            self.fc_norm = norm_layer(embed_dim)   # replaces `norm` (reference :27-32)
        else:
            self.norm = norm_layer(embed_dim)
        self.head = nn.Linear(embed_dim, num_classes) if num_classes > 0 else nn.Identity()
        self.init_weights()

    def init_weights(self):
        nn.init.trunc_normal_(self.pos_embed, std=.02)
        nn.init.trunc_normal_(self.cls_token, std=.02)
        for m in self.modules():
            if isinstance(m, nn.Linear):
                nn.init.trunc_normal_(m.weight, std=.02)
                if m.bias is not None:
                    nn.init.zeros_(m.bias)
            elif isinstance(m, nn.LayerNorm):
                nn.init.ones_(m.weight)
                nn.init.zeros_(m.bias)

    @torch.jit.ignore
    def no_weight_decay(self):
        return {"pos_embed", "cls_token"}

    def forward_features(self, x, drop_scales=None):
        """-> operand-type [B, D] features.  drop_scales: fixed stochastic-depth factors, fp32 [depth, 2, B]
        (engine.run_blocks); None draws them in training mode."""
        self._prepare()
        pe = self.patch_embed
        assert tuple(x.shape[2:]) == tuple(pe.img_size), "input size mismatch"
        eps = (self.fc_norm if self.global_pool else self.norm).eps
        tok = PatchEmbedFn.apply(x.float(), pe.proj.weight, pe.proj.bias, self.cls_token, self.pos_embed, None,
                                 pe.num_patches, pe.patch_size[0], self.dtype_, self.sink(), self._lp)
        tok, _ = self._blocks(self.blocks, tok, self.num_heads, eps, drop_scales=drop_scales)
        if self.global_pool:
            pooled = tok[:, 1:, :].mean(dim=1)  # global pool without cls token
            return self._ln(pooled, self.fc_norm)
        return self._ln(tok[:, 0].contiguous(), self.norm)  # LayerNorm is per token: the cls row alone

    _HEADS = ("nn.Linear", "nn.Identity", "nn.Sequential(nn.BatchNorm1d(affine=False), nn.Linear)")

    def _head(self, x):
        head = self.head
        if isinstance(head, nn.Identity):
            return x.float()
        if isinstance(head, nn.Linear):
            return self._linear(x, head, out_dtype=torch.float32)
        if isinstance(head, nn.Sequential) and len(head) == 2 and type(head[0]) is nn.BatchNorm1d \
                and not head[0].affine and isinstance(head[1], nn.Linear):
            # the linear probe's head (reference main_linprobe.py:222): training mode normalises with the batch
            # statistics and updates the running ones, eval() uses the running ones
            from ...resnet_engine import BatchNormFn
            x = BatchNormFn.apply(x.contiguous(), None, None, None, head[0], False, self.sink())
            return self._linear(x, head[1], out_dtype=torch.float32)
        raise TypeError(f"VisionTransformer.head must be one of {', '.join(self._HEADS)}; got {head!r}")

    def forward_head(self, feats):
        """`head` on given [B, D] features (what forward_features returns) -> fp32 logits"""
        self._prepare()
        return self._head(feats if feats.dtype == self.dtype_ else feats.to(self.dtype_))

    def forward(self, x, drop_scales=None):
        return self._head(self.forward_features(x, drop_scales=drop_scales))


def _vit(embed_dim, depth, num_heads, patch_size=16, **kwargs):
    return VisionTransformer(patch_size=patch_size, embed_dim=embed_dim, depth=depth, num_heads=num_heads, mlp_ratio=4,
                             qkv_bias=True, norm_layer=partial(nn.LayerNorm, eps=1e-6), **kwargs)


def vit_base_patch16(**kwargs):
    return _vit(768, 12, 12, **kwargs)


def vit_large_patch16(**kwargs):
    return _vit(1024, 24, 16, **kwargs)


def vit_huge_patch14(**kwargs):
    raise NotImplementedError("vit_huge_patch14: attention at head dimension 80 and 14-pixel patches are not built "
                              "(DESIGN.md §8)")
