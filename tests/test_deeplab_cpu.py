"""CPU: DeepLabV3Plus' module tree, refusals and bindings, and a guard on the checker (tests/deeplab_checks.py)."""
import os
import re

import pytest
import torch
import torch.nn.functional as F

import deeplab_checks as chk
from ssl4gie_amd import _lib, ops
from ssl4gie_amd.Models.deeplab import DeepLabV3Plus

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = {"ssl4gie_im2col3x3_dil", "ssl4gie_dwconv3x3_fwd", "ssl4gie_dwconv3x3_wgrad_workspace_bytes",
               "ssl4gie_dwconv3x3_wgrad", "ssl4gie_bilinear_up_ac_fwd", "ssl4gie_bilinear_up_ac_bwd", "ssl4gie_chan_copy"}


def _model(**kw):
    return DeepLabV3Plus("resnet50", encoder_weights=None, **kw)


@pytest.mark.parametrize("classes", [1, 3])
def test_state_dict_keys_and_shapes(classes):
    """smp 0.3.2's key -> shape table: every decoder and head key, the encoder's = torchvision ResNet50 minus fc.*"""
    sd = _model(classes=classes).state_dict()
    want = {"encoder." + k: v for k, v in chk.resnet50_key_shapes().items()}
    want.update(chk.decoder_key_shapes(classes))
    assert set(sd) == set(want), set(sd) ^ set(want)
    for k, v in sd.items():
        assert tuple(v.shape) == want[k], (k, tuple(v.shape), want[k])
    assert not any(k.startswith("encoder.fc.") for k in sd)
    assert sum(k.endswith("num_batches_tracked") for k in sd) == 53 + 9   # every BatchNorm: trunk + decoder


def test_layer4_is_dilated_and_the_rest_is_not():
    enc = _model().encoder
    for name, m in enc.named_modules():
        if isinstance(m, torch.nn.Conv2d) and name.startswith("layer4"):
            assert m.stride == (1, 1) and m.dilation == (2, 2), name
            assert m.padding == ((2, 2) if m.kernel_size == (3, 3) else (0, 0)), name
        elif isinstance(m, torch.nn.Conv2d):
            assert m.dilation == (1, 1), name
    assert enc.layer3[0].conv2.stride == (2, 2)
    dec = _model(decoder_atrous_rates=(6, 12, 18)).decoder
    assert [dec.aspp[0].convs[i][0][0].dilation[0] for i in (1, 2, 3)] == [6, 12, 18]


def test_encoder_load_state_dict_drops_fc():
    m = _model()
    sd = {k: torch.randn(v.shape) if v.is_floating_point() else v.clone() for k, v in m.encoder.state_dict().items()}
    whole = dict(sd, **{"fc.weight": torch.zeros(1000, 2048), "fc.bias": torch.zeros(1000)})
    res = m.encoder.load_state_dict(whole)
    assert not res.missing_keys and not res.unexpected_keys and "fc.weight" in whole
    assert torch.equal(m.encoder.layer4[2].conv3.weight, sd["layer4.2.conv3.weight"])


@pytest.mark.parametrize("kw", [dict(encoder_name="resnet34"), dict(encoder_name="resnet101"), dict(encoder_depth=4),
                                dict(encoder_output_stride=8), dict(in_channels=1), dict(activation="sigmoid"),
                                dict(aux_params=dict(classes=2)), dict(encoder_weights="imagenet")])
def test_refusals(kw):
    args = dict(encoder_name="resnet50", encoder_weights=None)
    args.update(kw)
    with pytest.raises(NotImplementedError) as e:
        DeepLabV3Plus(**args)
    if "encoder_weights" in kw:
        assert "encoder_weights=None" in str(e.value) and "encoder.load_state_dict" in str(e.value)


def test_default_signature_is_smp_s():
    import inspect
    sig = inspect.signature(DeepLabV3Plus.__init__)
    got = {k: p.default for k, p in sig.parameters.items() if k != "self"}
    assert got == dict(encoder_name="resnet34", encoder_depth=5, encoder_weights="imagenet", encoder_output_stride=16,
                       decoder_channels=256, decoder_atrous_rates=(12, 24, 36), in_channels=3, classes=1,
                       activation=None, upsampling=4, aux_params=None)
    with pytest.raises(NotImplementedError):
        DeepLabV3Plus()   # smp's defaults name resnet34 and a download


def test_input_shape_check():
    with pytest.raises(RuntimeError, match="divisible by 16"):
        _model()(torch.zeros(1, 3, 72, 64))


def test_initialisation():
    m = _model(classes=2).requires_grad_(False)
    w = m.decoder.block1[0].weight
    bound = (6.0 / 256) ** 0.5   # kaiming_uniform_, fan_in = 256, gain sqrt(2): sqrt(3) * sqrt(2 / fan_in)
    assert float(w.abs().max()) <= bound and float(w.abs().max()) > 0.9 * bound
    assert all(float((b.weight - 1).abs().max()) == 0 and float(b.bias.abs().max()) == 0
               for b in m.decoder.modules() if isinstance(b, torch.nn.BatchNorm2d))
    h = m.segmentation_head[0]
    assert float(h.bias.abs().max()) == 0 and float(h.weight.abs().max()) <= (6.0 / (256 + 2)) ** 0.5


def test_header_prototypes_and_abi():
    txt = open(os.path.join(ROOT, "include", "ssl4gie_hip.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    names = set(re.findall(r"\b(ssl4gie_[a-z0-9_]+)\s*\(", txt))
    assert names == set(_lib.PROTOTYPES), names ^ set(_lib.PROTOTYPES)
    assert NEW_SYMBOLS <= names
    assert _lib.ABI_VERSION == 13 and "return 13" in open(os.path.join(ROOT, "ssl4gie_amd", "csrc", "engine.hip")).read()


def test_workspace_query_and_cpu_refusals():
    L = _lib.load()
    assert L.ssl4gie_abi_version() == 13
    n = L.ssl4gie_dwconv3x3_wgrad_workspace_bytes(_lib.BF16, 2, 14, 14, 2048)
    assert n > 0 and n % (9 * 2048 * 4) == 0
    assert L.ssl4gie_dwconv3x3_wgrad_workspace_bytes(_lib.BF16, 2, 14, 14, 12) == 0   # C % 8
    x = torch.zeros(1, 4, 4, 8)
    w = torch.zeros(8, 1, 3, 3)
    for call in (lambda: ops.im2col3x3_dil(x, 2), lambda: ops.dwconv3x3_fwd(x, w, 2), lambda: ops.dwconv3x3_wgrad(x, x, 2),
                 lambda: ops.bilinear_up_ac_fwd(x, 4), lambda: ops.bilinear_up_ac_bwd(x, 4),
                 lambda: ops.chan_read(x, 0, 4)):
        with pytest.raises(RuntimeError, match="HIP device"):
            call()
    # the library validates before it launches: no GPU is needed to be refused
    assert L.ssl4gie_dwconv3x3_fwd(16, 16, 32, _lib.BF16, 1, 4, 4, 12, 1, 0, None) == 1000     # C % 8
    assert L.ssl4gie_dwconv3x3_fwd(16, 16, 32, _lib.BF16, 1, 4, 4, 8, 0, 0, None) == 1000      # dilation < 1
    assert L.ssl4gie_im2col3x3_dil(16, 32, _lib.BF16, 1, 4, 4, 8, 2, 64, None) == 1000         # ld < 9 C
    assert L.ssl4gie_bilinear_up_ac_fwd(16, 32, _lib.F32, 1, 4, 4, 1, 1, None) == 1000         # scale < 2
    assert L.ssl4gie_chan_copy(16, 4, 32, 8, _lib.F32, 4, 8, 1, None) == 1000                  # lds < C


@pytest.mark.parametrize("dil", [1, 2, 12])
def test_checker_depthwise_is_a_nine_tap_sum(dil):
    """guard on the checker: F.conv2d(groups = C, dilation) is the explicit tap sum the kernels are written from"""
    g = torch.Generator().manual_seed(dil)
    x = torch.randn(2, 16, 7, 9, generator=g, dtype=torch.float64)
    w = torch.randn(16, 1, 3, 3, generator=g, dtype=torch.float64)
    want = F.conv2d(x, w, padding=dil, dilation=dil, groups=16)
    assert float((chk.dwconv_taps(x, w, dil) - want).abs().max()) <= 1e-13
