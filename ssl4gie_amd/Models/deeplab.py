"""DeepLabV3+ (ResNet50, output stride 16) on the MI355X engine with segmentation_models_pytorch 0.3.2's module tree and
state_dict names: the import switch for `smp.DeepLabV3Plus(encoder_name="resnet50", ...)` of the reference's
Binary_segmentation/train_segmentation.py:153,166,173, eval_segmentation.py and predict_segmentation.py.

smp is neither vendored nor installed, so this restates, from its published source,
  * encoders/resnet.py + encoders/_utils.py: torchvision's ResNet50 without `fc`; `make_dilated(output_stride=16)` turns
    every convolution of layer4 into stride 1 / dilation 2 (3x3: padding 2); features = the layer1 and layer4 maps;
  * decoders/deeplabv3/decoder.py: DeepLabV3PlusDecoder — ASPP(2048 -> 256, separable=True) -> SeparableConv2d 3x3 ->
    BatchNorm -> ReLU -> x4 (align_corners=True); block1 (1x1, 256 -> 48) on the layer1 map; cat; block2 (separable 3x3,
    304 -> 256);
  * base/heads.py: SegmentationHead = Conv2d(256, classes, 1) -> UpsamplingBilinear2d(4) -> Identity;
  * base/initialization.py: kaiming_uniform_(fan_in, relu) / BatchNorm 1, 0 for the decoder, xavier_uniform_ for the head.
The nn.Conv2d / nn.BatchNorm2d children only hold parameters and buffers; the arithmetic runs on libssl4gie_hip.so
(`ssl4gie_amd.atrous_engine`, `resnet_engine`, `engine`), channels-last.  There is no torch path: a missing kernel raises.
"""
from __future__ import annotations

import torch
import torch.nn as nn

from ..atrous_engine import (ConcatFn, DepthwiseConv3x3Fn, DilatedConv3x3Fn, FanOutFn, PointwisePadFn, SegHeadACFn,
                             UpsampleACFn)
from ..conv_plan import k_pad
from ..dpt_engine import ForkFn
from ..engine import EngineModule, LinearFn
from ..resnet_engine import AvgPoolFn, BatchNormFn
from .resnet import ResNet50


class DilatedResNet50Encoder(ResNet50):
    """smp's ResNetEncoder("resnet50") after make_dilated(16): layer4 at stride 1, dilation 2; no `fc`, no `avgpool`."""

    out_channels = (3, 64, 256, 512, 1024, 2048)

    def __init__(self):
        super().__init__()
        self._low = None
        del self.avgpool
        for m in self.layer4.modules():
            if isinstance(m, nn.Conv2d):   # encoders/_utils.py replace_strides_with_dilation(module, 2)
                m.stride, m.dilation = (1, 1), (2, 2)
                m.padding = ((m.kernel_size[0] // 2) * 2,) * 2
            elif hasattr(m, "stride") and hasattr(m, "conv2"):
                m.stride = 1

    def load_state_dict(self, state_dict, **kwargs):
        sd = dict(state_dict)   # the reference passes whole ResNet50 dictionaries (train_segmentation.py:154-155)
        sd.pop("fc.bias", None)
        sd.pop("fc.weight", None)
        return super().load_state_dict(sd, **kwargs)

    def _c3(self, x, conv):
        if conv.dilation[0] == 1:
            return super()._c3(x, conv)
        return DilatedConv3x3Fn.apply(x, conv.weight, conv.dilation[0], self.sink(), self.lp_cache, True)

    def _block(self, x, blk):
        if blk is self.layer2[0]:   # the layer1 map also feeds the decoder's block1: fork it in front of layer2
            if torch.is_grad_enabled() and x.requires_grad:
                x, self._low = ForkFn.apply(x)
            else:
                self._low = x
        return super()._block(x, blk)

    def features(self, imgs):
        """-> (layer1 map [B, H/4, W/4, 256], layer4 map [B, H/16, W/16, 2048]), channels-last"""
        x4 = self.forward_maps(imgs)
        low, self._low = self._low, None
        return low, x4


def _separable(cin, cout, dilation):
    """smp SeparableConv2d(cin, cout, 3, padding = dilation, dilation, bias=False): [0] depthwise, [1] pointwise"""
    return nn.Sequential(nn.Conv2d(cin, cin, 3, 1, dilation, dilation, groups=cin, bias=False),
                         nn.Conv2d(cin, cout, 1, bias=False))


class ASPP(nn.Module):
    def __init__(self, cin, cout, rates):
        super().__init__()
        convs = [nn.Sequential(nn.Conv2d(cin, cout, 1, bias=False), nn.BatchNorm2d(cout), nn.ReLU())]
        for r in rates:
            convs.append(nn.Sequential(_separable(cin, cout, r), nn.BatchNorm2d(cout), nn.ReLU()))
        convs.append(nn.Sequential(nn.AdaptiveAvgPool2d(1), nn.Conv2d(cin, cout, 1, bias=False), nn.BatchNorm2d(cout),
                                   nn.ReLU()))
        self.convs = nn.ModuleList(convs)
        self.project = nn.Sequential(nn.Conv2d(len(convs) * cout, cout, 1, bias=False), nn.BatchNorm2d(cout), nn.ReLU(),
                                     nn.Dropout(0.5))


class DeepLabV3PlusDecoder(nn.Module):
    def __init__(self, cin, c_high, cout, rates):
        super().__init__()
        self.aspp = nn.Sequential(ASPP(cin, cout, rates), _separable(cout, cout, 1), nn.BatchNorm2d(cout), nn.ReLU())
        self.up = nn.UpsamplingBilinear2d(scale_factor=4)
        self.block1 = nn.Sequential(nn.Conv2d(c_high, 48, 1, bias=False), nn.BatchNorm2d(48), nn.ReLU())
        self.block2 = nn.Sequential(_separable(48 + cout, cout, 1), nn.BatchNorm2d(cout), nn.ReLU())
        self.out_channels = cout


class DeepLabV3Plus(EngineModule):
    """`smp.DeepLabV3Plus` signature; built for encoder_name="resnet50", encoder_depth=5, encoder_output_stride=16,
    in_channels=3, activation=None, aux_params=None (anything else raises NotImplementedError).
    forward(imgs fp32 [B, 3, H, W], H and W multiples of 16) -> fp32 logits [B, classes, H, W]."""

    def __init__(self, encoder_name="resnet34", encoder_depth=5, encoder_weights="imagenet", encoder_output_stride=16,
                 decoder_channels=256, decoder_atrous_rates=(12, 24, 36), in_channels=3, classes=1, activation=None,
                 upsampling=4, aux_params=None):
        super().__init__()
        for name, got, want in (("encoder_name", encoder_name, "resnet50"), ("encoder_depth", encoder_depth, 5),
                                ("encoder_output_stride", encoder_output_stride, 16), ("in_channels", in_channels, 3),
                                ("activation", activation, None), ("aux_params", aux_params, None)):
            if got != want:
                raise NotImplementedError(f"DeepLabV3Plus on the engine is built for {name}={want!r}, got {got!r}")
        if encoder_weights is not None:
            raise NotImplementedError(
                f"encoder_weights={encoder_weights!r}: there is no download; pass encoder_weights=None and call "
                "model.encoder.load_state_dict(...) with a ResNet50 dictionary")
        rates = tuple(int(r) for r in decoder_atrous_rates)
        if len(rates) != 3 or min(rates) < 1:
            raise ValueError(f"decoder_atrous_rates: three rates >= 1, got {decoder_atrous_rates!r}")
        if decoder_channels % 8 or int(classes) < 1 or int(upsampling) != upsampling or upsampling < 1:
            raise NotImplementedError(f"decoder_channels % 8 == 0, classes >= 1 and an integer upsampling >= 1, got "
                                      f"{decoder_channels}, {classes}, {upsampling}")
        self.encoder = self.adopt(DilatedResNet50Encoder())
        self.decoder = DeepLabV3PlusDecoder(2048, 256, decoder_channels, rates)
        self.segmentation_head = nn.Sequential(
            nn.Conv2d(decoder_channels, classes, 1),
            nn.UpsamplingBilinear2d(scale_factor=upsampling) if upsampling > 1 else nn.Identity(), nn.Identity())
        self.classification_head = None
        self.name = "deeplabv3plus-resnet50"
        for m in self.decoder.modules():   # smp base/initialization.py initialize_decoder
            if isinstance(m, nn.Conv2d):
                nn.init.kaiming_uniform_(m.weight, mode="fan_in", nonlinearity="relu")
            elif isinstance(m, nn.BatchNorm2d):
                nn.init.constant_(m.weight, 1)
                nn.init.constant_(m.bias, 0)
        nn.init.xavier_uniform_(self.segmentation_head[0].weight)   # initialize_head
        nn.init.constant_(self.segmentation_head[0].bias, 0)

    # ------------------------------------------------------------------ engine forward
    def _c1(self, x, conv):
        """1x1 convolution without bias -> (map, BatchNorm partial statistics of the map or None)"""
        y, st = LinearFn.apply(x.reshape(-1, x.shape[-1]), conv.weight, None, self.dtype_, self.dtype_, self.sink(),
                               self.lp_cache, True)
        return y.view(*x.shape[:-1], -1), st

    def _bn_relu(self, x, bn, stats=None):
        return BatchNormFn.apply(x, bn.weight, bn.bias, None, bn, True, self.sink(), stats)

    def _sep_bn_relu(self, x, sep, bn):
        """SeparableConv2d -> BatchNorm -> ReLU; x may carry zero pad channels behind the separable's own"""
        dw = DepthwiseConv3x3Fn.apply(x, sep[0].weight, sep[0].dilation[0], self.sink(), self.lp_cache)
        if x.shape[-1] != sep[1].weight.shape[1]:
            y, st = PointwisePadFn.apply(dw, sep[1].weight, self.sink(), self.lp_cache)
        else:
            y, st = self._c1(dw, sep[1])
        return self._bn_relu(y, bn, st)

    def _aspp(self, x4, aspp: ASPP):
        taps = FanOutFn.apply(x4, len(aspp.convs))
        y, st = self._c1(taps[0], aspp.convs[0][0])
        parts = [self._bn_relu(y, aspp.convs[0][1], st)]
        for t, br in zip(taps[1:-1], list(aspp.convs)[1:-1]):
            parts.append(self._sep_bn_relu(t, br[0], br[1]))
        pool = aspp.convs[-1]   # AdaptiveAvgPool2d(1) -> 1x1 -> BatchNorm over the B pooled rows -> ReLU -> broadcast
        p, st = self._c1(AvgPoolFn.apply(taps[-1]).to(self.dtype_), pool[1])
        parts.append(self._bn_relu(p, pool[2], st))
        y, st = self._c1(ConcatFn.apply(*parts), aspp.project[0])
        y = self._bn_relu(y, aspp.project[1], st)
        return nn.functional.dropout(y, aspp.project[3].p, self.training)

    def decode(self, x1, x4):
        d = self.decoder
        y = self._aspp(x4, d.aspp[0])
        y = self._sep_bn_relu(y, d.aspp[1], d.aspp[2])
        y = UpsampleACFn.apply(y, 4)
        h, st = self._c1(x1, d.block1[0])
        h = self._bn_relu(h, d.block1[1], st)
        parts = [y, h]
        width = y.shape[-1] + h.shape[-1]   # 304: no whole number of the bf16 GEMM's 64-deep K-tiles -> zero pad channels
        if k_pad(width, self.dtype_) != width:
            parts.append(torch.zeros(y.shape[0], k_pad(width, self.dtype_) - width, dtype=y.dtype, device=y.device))
        return self._sep_bn_relu(ConcatFn.apply(*parts), d.block2[0], d.block2[1])

    def forward(self, imgs):
        h, w = imgs.shape[-2:]
        if h % 16 or w % 16:   # smp base/model.py check_input_shape
            raise RuntimeError(f"Wrong input shape height={h}, width={w}. Expected image height and width divisible "
                               f"by 16. Consider pad your images to shape ({(h + 15) // 16 * 16}, {(w + 15) // 16 * 16}).")
        self._prepare()
        x1, x4 = self.encoder.features(imgs)
        y = self.decode(x1, x4)
        head = self.segmentation_head
        scale = int(head[1].scale_factor) if isinstance(head[1], nn.UpsamplingBilinear2d) else 1
        return SegHeadACFn.apply(y, head[0].weight, head[0].bias, scale, self.sink(), self.lp_cache)
