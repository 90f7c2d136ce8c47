"""Checker for DeepLabV3+ (tests/test_deeplab_cpu.py, test_gpu_atrous_kernels.py, test_gpu_deeplab.py): the model of
segmentation_models_pytorch 0.3.2 `DeepLabV3Plus(encoder_name="resnet50")` restated in plain torch ops on a state_dict
with smp's key names.  TEST INFRASTRUCTURE.

smp is installed nowhere and the reference vendors none of it, so parity is UNPINNED at this boundary: the restatement
follows smp's published source (encoders/resnet.py, encoders/_utils.py make_dilated, decoders/deeplabv3/decoder.py,
base/heads.py) and is anchored only by torch op semantics: F.conv2d with dilation / groups, F.batch_norm, F.interpolate,
F.adaptive_avg_pool2d.  It runs in whatever type the state_dict and the images have (fp64 for references).
"""
from __future__ import annotations

import functools

import torch
import torch.nn.functional as F

LAYERS = ((64, 3, 1, 1), (128, 4, 2, 1), (256, 6, 2, 1), (512, 3, 1, 2))   # planes, blocks, stride, dilation (stride 16)
RATES = (12, 24, 36)
RES_GAMMA = 0.1


def decoder_key_shapes(classes=1, ch=256, cin=2048, c_high=256):
    """every key of `decoder.*` and `segmentation_head.*` -> shape (smp 0.3.2)"""
    t = {}

    def bn(p, c):
        t.update({p + ".weight": (c,), p + ".bias": (c,), p + ".running_mean": (c,), p + ".running_var": (c,),
                  p + ".num_batches_tracked": ()})
    a = "decoder.aspp.0."
    t[a + "convs.0.0.weight"] = (ch, cin, 1, 1)
    bn(a + "convs.0.1", ch)
    for i in (1, 2, 3):
        t[a + f"convs.{i}.0.0.weight"] = (cin, 1, 3, 3)
        t[a + f"convs.{i}.0.1.weight"] = (ch, cin, 1, 1)
        bn(a + f"convs.{i}.1", ch)
    t[a + "convs.4.1.weight"] = (ch, cin, 1, 1)
    bn(a + "convs.4.2", ch)
    t[a + "project.0.weight"] = (ch, 5 * ch, 1, 1)
    bn(a + "project.1", ch)
    t["decoder.aspp.1.0.weight"] = (ch, 1, 3, 3)
    t["decoder.aspp.1.1.weight"] = (ch, ch, 1, 1)
    bn("decoder.aspp.2", ch)
    t["decoder.block1.0.weight"] = (48, c_high, 1, 1)
    bn("decoder.block1.1", 48)
    t["decoder.block2.0.0.weight"] = (48 + ch, 1, 3, 3)
    t["decoder.block2.0.1.weight"] = (ch, 48 + ch, 1, 1)
    bn("decoder.block2.1", ch)
    t["segmentation_head.0.weight"] = (classes, ch, 1, 1)
    t["segmentation_head.0.bias"] = (classes,)
    return t


def resnet50_key_shapes():
    """torchvision ResNet50's state_dict without fc.*: key -> shape"""
    t = {"conv1.weight": (64, 3, 7, 7)}

    def bn(p, c):
        t.update({p + ".weight": (c,), p + ".bias": (c,), p + ".running_mean": (c,), p + ".running_var": (c,),
                  p + ".num_batches_tracked": ()})
    bn("bn1", 64)
    cin = 64
    for li, (planes, blocks, _, _) in enumerate(LAYERS, start=1):
        for j in range(blocks):
            p = f"layer{li}.{j}"
            t[p + ".conv1.weight"] = (planes, cin, 1, 1)
            bn(p + ".bn1", planes)
            t[p + ".conv2.weight"] = (planes, planes, 3, 3)
            bn(p + ".bn2", planes)
            t[p + ".conv3.weight"] = (4 * planes, planes, 1, 1)
            bn(p + ".bn3", 4 * planes)
            if j == 0:
                t[p + ".downsample.0.weight"] = (4 * planes, cin, 1, 1)
                bn(p + ".downsample.1", 4 * planes)
            cin = 4 * planes
    return t


# ------------------------------------------------------------------ the restatement
def _bn(sd, p, x, training):
    """nn.BatchNorm2d: in training mode the running statistics IN `sd` are updated in place, as the module's are"""
    return F.batch_norm(x, sd[p + ".running_mean"], sd[p + ".running_var"], sd[p + ".weight"], sd[p + ".bias"],
                        training, 0.1, 1e-5)


def _bottleneck(sd, p, x, stride, dil, has_down, training):
    out = F.relu(_bn(sd, p + ".bn1", F.conv2d(x, sd[p + ".conv1.weight"]), training))
    out = F.conv2d(out, sd[p + ".conv2.weight"], stride=stride, padding=dil, dilation=dil)
    out = F.relu(_bn(sd, p + ".bn2", out, training))
    out = _bn(sd, p + ".bn3", F.conv2d(out, sd[p + ".conv3.weight"]), training)
    idn = x
    if has_down:
        idn = _bn(sd, p + ".downsample.1", F.conv2d(x, sd[p + ".downsample.0.weight"], stride=stride), training)
    return F.relu(out + idn)


def encoder(sd, imgs, training=True, prefix="encoder."):
    """-> (layer1 map, layer4 map), NCHW; layer4 at stride 1 / dilation 2"""
    sd = _Prefixed(sd, prefix)
    x = F.conv2d(imgs, sd["conv1.weight"], stride=2, padding=3)
    x = F.max_pool2d(F.relu(_bn(sd, "bn1", x, training)), 3, 2, 1)
    low = None
    for li, (planes, blocks, stride, dil) in enumerate(LAYERS, start=1):
        for j in range(blocks):
            x = _bottleneck(sd, f"layer{li}.{j}", x, stride if j == 0 else 1, dil, j == 0, training)
        if li == 1:
            low = x
    return low, x


class _Prefixed:
    def __init__(self, sd, prefix):
        self.sd, self.prefix = sd, prefix

    def __getitem__(self, k):
        return self.sd[self.prefix + k]


def _separable(sd, p, x, dil):
    c = x.shape[1]
    x = F.conv2d(x, sd[p + ".0.weight"], padding=dil, dilation=dil, groups=c)
    return F.conv2d(x, sd[p + ".1.weight"])


def decoder(sd, low, high, training=True, dropout_p=0.0, rates=RATES):
    a = "decoder.aspp.0."
    size = high.shape[-2:]
    parts = [F.relu(_bn(sd, a + "convs.0.1", F.conv2d(high, sd[a + "convs.0.0.weight"]), training))]
    for i, r in enumerate(rates, start=1):
        parts.append(F.relu(_bn(sd, a + f"convs.{i}.1", _separable(sd, a + f"convs.{i}.0", high, r), training)))
    p = F.conv2d(F.adaptive_avg_pool2d(high, 1), sd[a + "convs.4.1.weight"])
    p = F.relu(_bn(sd, a + "convs.4.2", p, training))
    parts.append(F.interpolate(p, size=size, mode="bilinear", align_corners=False))
    y = F.conv2d(torch.cat(parts, dim=1), sd[a + "project.0.weight"])
    y = F.dropout(F.relu(_bn(sd, a + "project.1", y, training)), dropout_p, training)
    y = F.relu(_bn(sd, "decoder.aspp.2", _separable(sd, "decoder.aspp.1", y, 1), training))
    y = F.interpolate(y, scale_factor=4, mode="bilinear", align_corners=True)
    h = F.relu(_bn(sd, "decoder.block1.1", F.conv2d(low, sd["decoder.block1.0.weight"]), training))
    y = _separable(sd, "decoder.block2.0", torch.cat([y, h], dim=1), 1)
    return F.relu(_bn(sd, "decoder.block2.1", y, training))


def deeplab(sd, imgs, training=True, dropout_p=0.0, upsampling=4):
    """logits [B, classes, H, W] of smp.DeepLabV3Plus("resnet50", encoder_output_stride=16) on the state_dict `sd`"""
    low, high = encoder(sd, imgs, training)
    y = decoder(sd, low, high, training, dropout_p)
    y = F.conv2d(y, sd["segmentation_head.0.weight"], sd["segmentation_head.0.bias"])
    return F.interpolate(y, scale_factor=upsampling, mode="bilinear", align_corners=True)


def dwconv_taps(x, w, dil):
    """the depthwise dilated 3x3 convolution (padding = dil) as an explicit nine-tap sum: x [B,C,H,W], w [C,1,3,3]"""
    B, C, H, W = x.shape
    xp = F.pad(x, (dil, dil, dil, dil))
    y = torch.zeros_like(x)
    for ky in range(3):
        for kx in range(3):
            y = y + w[:, 0, ky, kx].view(1, C, 1, 1) * xp[:, :, ky * dil:ky * dil + H, kx * dil:kx * dil + W]
    return y


# ------------------------------------------------------------------ the model cases of tests/test_gpu_deeplab.py
def model_weights(seed=5, **model_kw):
    """a state_dict for the engine model AND the restatement: the model's own initialisation, with every BatchNorm's
    affine pair and running statistics moved off 1 / 0 (identity statistics would hide a swapped or dropped term)"""
    from ssl4gie_amd.Models.deeplab import DeepLabV3Plus
    torch.manual_seed(seed)
    m = DeepLabV3Plus("resnet50", encoder_weights=None, **model_kw)
    g = torch.Generator().manual_seed(seed + 1)
    sd = {k: v.clone() for k, v in m.state_dict().items()}
    for k, v in sd.items():
        if k.endswith("running_mean") or (k.endswith(".bias") and v.dim() == 1):
            sd[k] = 0.2 * torch.randn(v.shape, generator=g)
        elif k.endswith("running_var") or (k.endswith(".weight") and v.dim() == 1):
            sd[k] = 0.5 + torch.rand(v.shape, generator=g)
    for k in sd:   # weak residual branches (MoCo's zero_init_residual starts them at 0): with gamma ~ 1 on bn3 a random
        if k.startswith("encoder.") and k.endswith("bn3.weight"):   # ResNet50 grows rounding by 1.3x per block
            sd[k] = sd[k] * RES_GAMMA
    return sd


def model_inputs(shape=(4, 3, 64, 64), seed=11):
    """images with clearly different global statistics (a per-image scale and offset): the ASPP pooling branch
    normalises over only B pooled rows, which on i.i.d. noise images are nearly equal — BatchNorm then amplifies
    rounding in ANY arithmetic.  Returns (imgs, wy): wy weights the logits into the scalar that is differentiated."""
    g = torch.Generator().manual_seed(seed)
    B = shape[0]
    imgs = torch.randn(shape, generator=g)
    scale = torch.linspace(0.5, 2.0, B).view(B, 1, 1, 1)
    offset = torch.linspace(-1.0, 1.0, B).view(B, 1, 1, 1)
    smooth = F.interpolate(torch.randn(B, 3, 4, 4, generator=g), size=shape[-2:], mode="bilinear", align_corners=True)
    imgs = (imgs + 2.0 * smooth) * scale + offset
    wy = torch.randn(B, 1, *shape[-2:], generator=g) / (shape[-1] * shape[-2])
    return imgs, wy


def run_restatement(sd, imgs, wy, dtype, training=True, autocast=False):
    """forward + backward of the restatement -> (logits, {key: gradient}, {key: running statistic after the step})"""
    flt = {k: (v.detach().clone().to(dtype) if v.is_floating_point() else v.clone()) for k, v in sd.items()}
    for k, v in flt.items():
        if v.is_floating_point() and not k.endswith(("running_mean", "running_var")):
            v.requires_grad_(training)
    x = imgs.to(dtype)
    with torch.autocast("cpu", torch.bfloat16, enabled=autocast), torch.set_grad_enabled(training):
        out = deeplab(flt, x, training)
    grads = {}
    if training:
        (out.to(dtype) * wy.to(dtype)).sum().backward()
        grads = {k: v.grad for k, v in flt.items() if v.requires_grad}
    stats = {k: v.detach() for k, v in flt.items() if k.endswith(("running_mean", "running_var"))}
    return out.detach(), grads, stats


@functools.lru_cache(maxsize=None)
def reference(shape=(4, 3, 64, 64), training=True):
    """the fp64 run (computed once, shared, never modified) and the restatement's own fp32 and bf16-autocast runs on
    the same weights and inputs -> dict(sd, imgs, wy, f64, f32, bf16) of (logits, grads, stats) triples"""
    sd = model_weights()
    imgs, wy = model_inputs(shape)
    out = dict(sd=sd, imgs=imgs, wy=wy, f64=run_restatement(sd, imgs, wy, torch.float64, training))
    out["f32"] = run_restatement(sd, imgs, wy, torch.float32, training)
    if training:
        out["bf16"] = run_restatement(sd, imgs, wy, torch.float32, training, autocast=True)
    return out
