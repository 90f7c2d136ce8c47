"""ResNet50 trunk on the MI355X engine with torchvision's module tree / state_dict names
(`conv1.weight, bn1.{weight,bias,running_mean,running_var,num_batches_tracked},
layer{1-4}.{j}.{conv1,bn1,conv2,bn2,conv3,bn3}.*, layer{k}.0.downsample.{0,1}.*`).

torchvision 0.10 is pinned by the reference (`requirements.txt:10`) but neither vendored nor
installed, so this restates `ResNet(Bottleneck, [3, 4, 6, 3])` (v1.5: the stride sits on the 3x3
convolution; kaiming-normal fan_out init; BN weight 1 / bias 0; `zero_init_residual` zeroes every
bn3.weight — used by MoCo, Models/moco_v3/main_moco.py:186).  The nn.Conv2d / nn.BatchNorm2d
children only hold parameters and buffers; the arithmetic runs on libssl4gie_hip.so
(`ssl4gie_amd.resnet_engine`), channels-last.
"""
from __future__ import annotations

import torch
import torch.nn as nn

from ..dpt_engine import Conv3x3Fn
from ..engine import EngineModule, GradJoin, LinearFn
from ..resnet_engine import (AvgPoolFn, BatchNormFn, BnReluMaxPoolFn, MaxPoolFn, StemConvFn, Subsample2Fn,
                             _count_batch, _sync_group, bn_relu_maxpool_ok, bn_trains)


class FrozenBatchNorm2d(nn.Module):
    """BatchNorm2d whose statistics AND affine parameters are fixed: torchvision 0.10's class of this name
    (`torchvision/ops/misc.py`; un-vendored and restated, see the module docstring), the norm layer of
    `fasterrcnn_resnet50_fpn`'s trunk (reference Object_detection/train_detection.py:197-202).  weight, bias,
    running_mean and running_var are buffers, there is no `num_batches_tracked`, no momentum and no training mode; the
    gradient still passes through the per-channel map y = (x - running_mean) rsqrt(running_var + eps) weight + bias.
    On the engine the arithmetic is resnet_engine.BatchNormFn's (`frozen_statistics` is what it looks for); `forward`
    is the torch formula on a plain NCHW tensor."""
    frozen_statistics = True

    def __init__(self, num_features, eps=1e-5):
        super().__init__()
        self.num_features, self.eps = num_features, eps
        self.register_buffer("weight", torch.ones(num_features))
        self.register_buffer("bias", torch.zeros(num_features))
        self.register_buffer("running_mean", torch.zeros(num_features))
        self.register_buffer("running_var", torch.ones(num_features))

    def _load_from_state_dict(self, state_dict, prefix, local_metadata, strict, missing_keys, unexpected_keys,
                              error_msgs):
        # an ordinary BatchNorm2d checkpoint loads with strict=True: its batch count has no home here
        state_dict.pop(prefix + "num_batches_tracked", None)
        super()._load_from_state_dict(state_dict, prefix, local_metadata, strict, missing_keys, unexpected_keys,
                                      error_msgs)

    def forward(self, x):
        scale = (self.weight * torch.rsqrt(self.running_var + self.eps)).reshape(1, -1, 1, 1)
        shift = self.bias.reshape(1, -1, 1, 1) - self.running_mean.reshape(1, -1, 1, 1) * scale
        return x * scale + shift

    def extra_repr(self):
        return f"{self.num_features}, eps={self.eps}"


class Bottleneck(nn.Module):
    expansion = 4

    def __init__(self, inplanes, planes, stride=1, downsample=None, norm_layer=None):
        super().__init__()
        norm_layer = norm_layer or nn.BatchNorm2d
        self.conv1 = nn.Conv2d(inplanes, planes, 1, bias=False)
        self.bn1 = norm_layer(planes)
        self.conv2 = nn.Conv2d(planes, planes, 3, stride, 1, bias=False)
        self.bn2 = norm_layer(planes)
        self.conv3 = nn.Conv2d(planes, planes * 4, 1, bias=False)
        self.bn3 = norm_layer(planes * 4)
        self.relu = nn.ReLU(inplace=True)
        self.downsample = downsample
        self.stride = stride


class ResNet50(EngineModule):
    """the trunk (`forward_maps` -> channels-last layer4 map, or the 4 stage maps; `pooled`) and, when built with
    num_classes, torchvision's `forward` through `fc`"""

    STAGES = ("conv1", "layer1", "layer2", "layer3", "layer4")   # `freeze_stages` counts them from the end

    def __init__(self, zero_init_residual=False, num_classes=None, norm_layer=None):
        """norm_layer: None (nn.BatchNorm2d) or a class with its constructor, e.g. FrozenBatchNorm2d"""
        super().__init__()
        self._norm_layer = norm_layer or nn.BatchNorm2d
        self._freeze_rule = False
        self.inplanes = 64
        self.conv1 = nn.Conv2d(3, 64, 7, 2, 3, bias=False)
        self.bn1 = self._norm_layer(64)
        self.relu = nn.ReLU(inplace=True)
        self.maxpool = nn.MaxPool2d(3, 2, 1)
        self.layer1 = self._make_layer(64, 3)
        self.layer2 = self._make_layer(128, 4, stride=2)
        self.layer3 = self._make_layer(256, 6, stride=2)
        self.layer4 = self._make_layer(512, 3, stride=2)
        self.avgpool = nn.AdaptiveAvgPool2d((1, 1))
        if num_classes is not None:  # torchvision's classifier slot (MoCo replaces it by its projector)
            self.fc = nn.Linear(2048, num_classes)
        for m in self.modules():
            if isinstance(m, nn.Conv2d):
                nn.init.kaiming_normal_(m.weight, mode="fan_out", nonlinearity="relu")
            elif isinstance(m, nn.BatchNorm2d):
                nn.init.constant_(m.weight, 1)
                nn.init.constant_(m.bias, 0)
        if zero_init_residual:
            for m in self.modules():
                if isinstance(m, Bottleneck):
                    nn.init.constant_(m.bn3.weight, 0)

    def _make_layer(self, planes, blocks, stride=1):
        downsample = None
        if stride != 1 or self.inplanes != planes * 4:
            downsample = nn.Sequential(nn.Conv2d(self.inplanes, planes * 4, 1, stride, bias=False),
                                       self._norm_layer(planes * 4))
        layers = [Bottleneck(self.inplanes, planes, stride, downsample, self._norm_layer)]
        self.inplanes = planes * 4
        for _ in range(1, blocks):
            layers.append(Bottleneck(self.inplanes, planes, norm_layer=self._norm_layer))
        return nn.Sequential(*layers)

    def freeze_stages(self, trainable_layers):
        """torchvision's rule of `resnet_fpn_backbone(trainable_layers=...)` (detection/backbone_utils.py; 5 is what
        the reference passes as trainable_backbone_layers): the last `trainable_layers` of conv1, layer1 .. layer4
        keep training, every parameter whose name starts with none of them is frozen.  (torchvision also names bn1
        at 5; under FrozenBatchNorm2d it has no parameters.)  From then on `forward_maps` runs the leading stages
        without a trainable parameter under torch.no_grad()."""
        if not isinstance(trainable_layers, int) or not 0 <= trainable_layers <= 5:
            raise ValueError(f"trainable_layers is {trainable_layers!r}: an integer from 0 to 5")
        train = self.STAGES[::-1][:trainable_layers]
        for name, p in self.named_parameters():
            if not name.startswith(train):
                p.requires_grad_(False)
        self._freeze_rule = True
        return self

    def _frozen_lead(self):
        """how many of (stem, layer1 .. layer4), from the input on, hold no trainable parameter — counted only
        after `freeze_stages`: these run under no_grad, so no activation is kept and no backward kernel runs"""
        if not self._freeze_rule:
            return 0
        n = 0
        for mods in ((self.conv1, self.bn1), (self.layer1,), (self.layer2,), (self.layer3,), (self.layer4,)):
            if any(p.requires_grad for m in mods for p in m.parameters()):
                break
            n += 1
        return n

    # ------------------------------------------------------------------ engine forward
    def _bn(self, x, bn, relu, res=None, stats=None, join=None):
        return BatchNormFn.apply(x, bn.weight, bn.bias, res, bn, relu, self.sink(), stats, join)

    def _c1(self, x, conv, join=None):
        """1x1 convolution -> (map, BatchNorm partial statistics of the map or None)"""
        if conv.stride[0] == 2:
            x = Subsample2Fn.apply(x, join)  # the pixel pick deposits its scattered gradient in the join
            join = None  # ... and sits between x and the GEMM: the GEMM's gradient is not x's
        B, H, W, C = x.shape
        y, st = LinearFn.apply(x.reshape(-1, C), conv.weight, None, self.dtype_, self.dtype_, self.sink(),
                               self.lp_cache, True, join)
        return y.view(B, H, W, -1), st

    def _c3(self, x, conv):
        """3x3 convolution (Bottleneck.conv2) -> (map, BatchNorm partial statistics of the map or None)"""
        return Conv3x3Fn.apply(x, conv.weight, None, conv.stride[0], False, self.sink(), self.lp_cache, True)

    def _c1_bn_nograd(self, x, conv, bn, relu, res=None):
        """1x1 convolution + training-mode BatchNorm (+ residual) (+ ReLU) when nothing is kept for a backward pass
        (torch.no_grad(): MoCo's momentum encoder, moco/builder.py:127-135) and the map gets WIDER (conv3,
        downsample: C -> 4C): the product runs twice — first for the batch statistics alone (colstats with C == NULL:
        nothing written), then with the normalisation, the residual add and the ReLU in its epilogue — instead of
        writing the raw 4C-wide map and re-reading it in a BatchNorm pass: 2.5 instead of 4.25 passes over that map.
        The statistics are those of the bf16-rounded raw outputs, as on the other path; the affine map is applied to
        the fp32 accumulators (one rounding less).  Returns None when the shapes do not qualify."""
        from .. import ops
        if conv.stride[0] == 2:
            x = ops.subsample2(x.contiguous())
        B, H, W, C = x.shape
        n_out = conv.weight.shape[0]
        x2 = x.reshape(-1, C)
        w, _ = self.lp_cache.get(conv.weight, self.dtype_)
        stats = ops.linear_colstats_only(x2, w)
        mom = bn.momentum if bn.momentum is not None else 0.1
        gd = bn.weight.detach() if bn.weight is not None else None
        bd = bn.bias.detach() if bn.bias is not None else None
        sync, group = _sync_group(bn)
        if sync:   # SyncBatchNorm: the statistics-only product's partials -> exchange -> global coefficients
            from ..resnet_engine import sync_batch_stats
            mean_l, var_l = ops.bn_stats_from_partials(stats, x2.shape[0])   # of the product's n_out columns
            mean, rstd, _ = sync_batch_stats(mean_l, var_l, x2.shape[0], bn, group)
            coef = ops.bn_coef_stats(mean, rstd, gd, bd)
        else:
            coef, _, _ = ops.bn_coef_partials(stats, x2.shape[0], gd, bd, bn.running_mean, bn.running_var, mom, bn.eps)
        if bn.num_batches_tracked is not None:
            _count_batch(bn)
        r2 = res.contiguous().view(-1, n_out) if res is not None else None
        return ops.linear_affine_fwd(x2, w, coef[0], coef[1], r2, relu).view(B, H, W, n_out)

    def _recompute_ok(self, x, conv, bn):
        from .. import ops
        if torch.is_grad_enabled() or self.dtype_ != torch.bfloat16:
            return False
        from ..resnet_engine import _SYNC_FUSED
        if not bn_trains(bn) or (_sync_group(bn)[0] and not _SYNC_FUSED):
            return False
        st = conv.stride[0]
        rows = x.shape[0] * ((x.shape[1] - 1) // st + 1) * ((x.shape[2] - 1) // st + 1)
        return conv.weight.shape[0] > conv.weight.shape[1] and \
            ops.colstats_ok(rows, conv.weight.shape[0], conv.weight.shape[1], self.dtype_)

    def _block(self, x, blk: Bottleneck):
        # every convolution hands the batch statistics of its output to the BatchNorm that follows
        # (column sums from the GEMM epilogue): no separate statistics pass over the maps
        # x feeds conv1 and the identity (or downsample) branch: one GradJoin, conv1 is the adder
        join = GradJoin.for_tensor(x)
        out, st = self._c1(x, blk.conv1, join)
        out = self._bn(out, blk.bn1, True, stats=st)
        out, st = self._c3(out, blk.conv2)
        out = self._bn(out, blk.bn2, True, stats=st)
        identity = x
        if blk.downsample is not None:
            if self._recompute_ok(x, blk.downsample[0], blk.downsample[1]):
                identity = self._c1_bn_nograd(x, blk.downsample[0], blk.downsample[1], False)
            else:
                idn, sti = self._c1(x, blk.downsample[0], join)
                identity = self._bn(idn, blk.downsample[1], False, stats=sti)
            join = None  # bn3's residual input is the downsample branch, not x
        if self._recompute_ok(out, blk.conv3, blk.bn3):
            return self._c1_bn_nograd(out, blk.conv3, blk.bn3, True, res=identity)
        out, st = self._c1(out, blk.conv3)
        return self._bn(out, blk.bn3, True, res=identity, stats=st, join=join)  # relu(bn3(out) + identity)

    def prepare_inputs(self, imgs):
        """build the per-batch stem operand (bf16: the packed image) on the CURRENT stream, so that two
        forward passes over the same batch on different streams only read it (moco/builder.py)"""
        from .. import ops
        from ..resnet_engine import STEM_COLS
        if imgs.dtype != torch.float32 or not imgs.is_contiguous():
            return  # StemConvFn makes its own copy: nothing is shared between the passes
        if self.dtype_ == torch.bfloat16 and self.conv1.weight.shape[0] == 64 and imgs.shape[1] == 3:
            STEM_COLS.get(imgs, self.dtype_, ops.stem7x7_pack)
        else:
            STEM_COLS.get(imgs, self.dtype_)   # the patch matrix (fp32 parity mode)

    def forward_maps(self, imgs, all_stages=False):
        self._prepare()
        lead = self._frozen_lead()   # after freeze_stages: the stages in front of the first trainable one
        with torch.set_grad_enabled(torch.is_grad_enabled() and lead < 1):
            x, st = StemConvFn.apply(imgs, self.conv1.weight, self.dtype_, self.sink(), self.lp_cache, True)
            if bn_relu_maxpool_ok(x, self.bn1, st):   # bn1 -> relu -> maxpool in one pass over the convolution output
                x = BnReluMaxPoolFn.apply(x, self.bn1.weight, self.bn1.bias, self.bn1, self.sink(), st)
            else:   # fixed statistics (evaluation mode, FrozenBatchNorm2d) take the separate passes
                x = self._bn(x, self.bn1, True, stats=st)
                x = MaxPoolFn.apply(x)
        maps = []
        for i, layer in enumerate((self.layer1, self.layer2, self.layer3, self.layer4)):
            with torch.set_grad_enabled(torch.is_grad_enabled() and lead < i + 2):
                for blk in layer:
                    x = self._block(x, blk)
            maps.append(x)
        return maps if all_stages else x

    def pooled(self, imgs):
        """[B, 2048] fp32: avgpool + flatten of the layer4 map"""
        return AvgPoolFn.apply(self.forward_maps(imgs))

    def forward(self, imgs):
        """torchvision's `ResNet.forward`: pooled features -> `fc` -> fp32 logits [B, num_classes] (the 'fc' arm of the
        linear probe, reference Models/moco_v3/main_lincls.py:157-161)"""
        if not isinstance(getattr(self, "fc", None), nn.Linear):
            raise RuntimeError("ResNet50.forward needs the classifier `fc`: build it with num_classes "
                               "(resnet50(num_classes=...)); a trunk built without one has pooled() / forward_maps()")
        x = self.pooled(imgs).to(self.dtype_)
        return LinearFn.apply(x, self.fc.weight, self.fc.bias, self.dtype_, torch.float32, self.sink(), self.lp_cache)


def resnet50(num_classes=1000, zero_init_residual=False, norm_layer=None, **kwargs):
    """torchvision.models.resnet50 signature subset used by the reference (main_moco.py:185-187; norm_layer:
    detection's FrozenBatchNorm2d trunk, Object_detection/train_detection.py:197-202)"""
    return ResNet50(zero_init_residual=zero_init_residual, num_classes=num_classes, norm_layer=norm_layer)
