"""CPU: the model side of frozen BatchNorm (Models/resnet.py: FrozenBatchNorm2d, norm_layer, freeze_stages), the
formula the GPU tests hold ssl4gie_bn_bwd_frozen to, and the entry point's argument validation.

The GPU module (tests/test_gpu_frozen_bn.py) takes its reference from `bn_checks.ref_backward(..., inv_count=1,
sums=zeros)`; `test_frozen_reference_formula_is_torch_autograd` pins that expression to fp64 autograd through
`F.batch_norm(training=False)`, so the kernels are compared with torch itself and with no formula of this project's.
The validation table below is written out from the header's description, not derived from the library; validation
runs before anything touches the device, so those calls need no GPU (combinations the table accepts would launch and
are NOT called)."""
import itertools

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import bn_checks as bc
from ssl4gie_amd import _lib
from ssl4gie_amd._lib import BF16, F32

F64 = torch.float64


def G(seed):
    return torch.Generator("cpu").manual_seed(seed)


# ===================================================================== FrozenBatchNorm2d
def test_frozen_batchnorm_has_buffers_and_no_parameters():
    from ssl4gie_amd.Models.resnet import FrozenBatchNorm2d
    m = FrozenBatchNorm2d(24)
    assert list(m.parameters()) == []
    assert [k for k, _ in m.named_buffers()] == ["weight", "bias", "running_mean", "running_var"]
    assert m.eps == 1e-5 and all(b.shape == (24,) for b in m.buffers())
    assert not hasattr(m, "momentum") and not hasattr(m, "num_batches_tracked")
    assert torch.equal(m.weight, torch.ones(24)) and torch.equal(m.running_var, torch.ones(24))
    assert not m.bias.any() and not m.running_mean.any()
    assert FrozenBatchNorm2d(8, eps=0.0).eps == 0.0


def test_ordinary_resnet50_checkpoint_loads_strictly_into_the_frozen_trunk():
    from ssl4gie_amd.Models.resnet import FrozenBatchNorm2d, ResNet50, resnet50
    torch.manual_seed(3)
    src = ResNet50()
    g = G(4)
    with torch.no_grad():
        for mod in src.modules():
            if isinstance(mod, nn.BatchNorm2d):
                for t in (mod.weight, mod.bias, mod.running_mean):
                    t.copy_(torch.randn(t.shape, generator=g))
                mod.running_var.copy_(0.5 + torch.rand(mod.running_var.shape, generator=g))
    sd = src.state_dict()
    dst = ResNet50(norm_layer=FrozenBatchNorm2d)
    res = dst.load_state_dict(sd, strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    tracked = {k for k in sd if k.endswith("num_batches_tracked")}
    assert len(tracked) == 53 and set(dst.state_dict()) == set(sd) - tracked
    assert all(torch.equal(v, sd[k]) for k, v in dst.state_dict().items())
    assert any(k.endswith("num_batches_tracked") for k in sd), "the caller's dict keeps its keys"
    assert sum(isinstance(m, FrozenBatchNorm2d) for m in dst.modules()) == 53
    assert not any(isinstance(m, nn.BatchNorm2d) for m in dst.modules())
    # the default is what it was: nn.BatchNorm2d everywhere, the same keys
    assert sum(isinstance(m, nn.BatchNorm2d) for m in src.modules()) == 53
    assert set(resnet50(num_classes=None).state_dict()) == set(sd)
    assert isinstance(resnet50(num_classes=None, norm_layer=FrozenBatchNorm2d).layer3[0].downsample[1], FrozenBatchNorm2d)
    assert not [n for n, _ in dst.named_parameters() if "bn" in n or "downsample.1" in n]


def test_frozen_batchnorm_forward_and_autograd_equal_torch_eval_batchnorm_fp64():
    from ssl4gie_amd.Models.resnet import FrozenBatchNorm2d
    g = G(5)
    C = 12
    m = FrozenBatchNorm2d(C).double()
    with torch.no_grad():
        m.weight.copy_(torch.randn(C, generator=g, dtype=F64))
        m.bias.copy_(torch.randn(C, generator=g, dtype=F64))
        m.running_mean.copy_(torch.randn(C, generator=g, dtype=F64))
        m.running_var.copy_(0.1 + torch.rand(C, generator=g, dtype=F64))
        m.weight[1] = 0.0
        m.weight[2] = -1.5
    m.train()    # the flag means nothing to it
    x = torch.randn(3, C, 5, 4, generator=g, dtype=F64)
    dy = torch.randn(3, C, 5, 4, generator=g, dtype=F64)
    xa, xb = x.clone().requires_grad_(True), x.clone().requires_grad_(True)
    ya = m(xa)
    yb = F.batch_norm(xb, m.running_mean, m.running_var, m.weight, m.bias, False, 0.1, m.eps)
    ya.backward(dy)
    yb.backward(dy)
    assert float((ya - yb).detach().abs().max()) <= 1e-14 * float(yb.detach().abs().max())
    assert float((xa.grad - xb.grad).abs().max()) <= 1e-14 * float(xb.grad.abs().max())
    assert not ya.requires_grad or all(not b.requires_grad for b in m.buffers())


# ===================================================================== freeze_stages
def _expected_trainable(names, k):
    train = ("layer4", "layer3", "layer2", "layer1", "conv1")[:k]
    return {n for n in names if any(n.startswith(t) for t in train)}


@pytest.mark.parametrize("frozen_bn", [True, False], ids=["FrozenBatchNorm2d", "BatchNorm2d"])
def test_freeze_stages_leaves_exactly_torchvisions_set_trainable(frozen_bn):
    from ssl4gie_amd.Models.resnet import FrozenBatchNorm2d, ResNet50
    for k in range(6):
        m = ResNet50(norm_layer=FrozenBatchNorm2d if frozen_bn else None, num_classes=None if frozen_bn else 10)
        names = [n for n, _ in m.named_parameters()]
        assert m.freeze_stages(k) is m
        got = {n for n, p in m.named_parameters() if p.requires_grad}
        assert got == _expected_trainable(names, k), (k, sorted(got ^ _expected_trainable(names, k)))
        # spelled out: the stage prefixes, and never bn1 / fc (which start with none of the five names)
        assert all(n.split(".")[0] in ("layer4", "layer3", "layer2", "layer1", "conv1")[:k] for n in got)
        assert ("conv1.weight" in got) == (k == 5) and ("layer4.2.conv3.weight" in got) == (k >= 1)
        assert ("layer2.0.downsample.0.weight" in got) == (k >= 3) and ("layer1.0.conv1.weight" in got) == (k >= 4)
        # the stages in front of the first trainable one run under no_grad: stem, layer1, ...
        lead = {0: 5, 1: 4, 2: 3, 3: 2, 4: 1, 5: 0}[k]
        assert m._frozen_lead() == lead, (k, m._frozen_lead())
    assert ResNet50(norm_layer=FrozenBatchNorm2d)._frozen_lead() == 0    # never without the rule


def test_freeze_stages_refuses_values_outside_0_to_5():
    from ssl4gie_amd.Models.resnet import FrozenBatchNorm2d, ResNet50
    m = ResNet50(norm_layer=FrozenBatchNorm2d)
    for bad in (-1, 6, 100, 2.5, None, "3"):
        with pytest.raises(ValueError):
            m.freeze_stages(bad)
    assert all(p.requires_grad for p in m.parameters())     # a refused call freezes nothing


# ===================================================================== the formula of the GPU tests
@pytest.mark.parametrize("relu", [False, True], ids=["id", "relu"])
@pytest.mark.parametrize("affine", [False, True], ids=["plain", "affine"])
def test_frozen_reference_formula_is_torch_autograd(relu, affine):
    """bn_checks.ref_backward with inv_count = 1 and zero sums IS the backward through F.batch_norm(training=False)"""
    g = G(11 + relu + 2 * affine)
    rows, C, eps = 37, 8, 1e-5
    x = torch.randn(rows, C, generator=g, dtype=F64) * 2 + 1
    dy = torch.randn(rows, C, generator=g, dtype=F64)
    mean = torch.randn(C, generator=g, dtype=F64)
    var = 0.2 + torch.rand(C, generator=g, dtype=F64)
    gamma = torch.randn(C, generator=g, dtype=F64).requires_grad_(True) if affine else None
    beta = torch.randn(C, generator=g, dtype=F64).requires_grad_(True) if affine else None
    if affine:
        with torch.no_grad():
            gamma[1], gamma[2] = 0.0, -gamma[2].abs() - 0.1
    xr = x.clone().requires_grad_(True)
    y = F.batch_norm(xr, mean, var, gamma, beta, False, 0.1, eps)
    if relu:
        y = F.relu(y)
    y.backward(dy)
    rstd = (var + eps) ** -0.5
    bw = bc.ref_backward(dy, (y.detach() > 0) if relu else None, x, mean, rstd,
                         gamma.detach() if affine else None, 1.0, torch.zeros(2, C, dtype=F64))
    scale = float(xr.grad.abs().max())
    assert float((bw["dx"] - xr.grad).abs().max()) <= 1e-14 * scale
    a = rstd * (gamma.detach() if affine else 1.0)
    assert torch.equal(bw["mag_dx"], a.abs() * bw["g"].abs())     # the bound's mag is |a| |g|
    if affine:
        assert float((bw["s1"] - beta.grad).abs().max()) <= 1e-13 * float(bw["A1"].max())
        assert float((bw["s2"] - gamma.grad).abs().max()) <= 1e-13 * float(bw["A2"].max())


# ===================================================================== argument validation of ssl4gie_bn_bwd_frozen
EARG = 1000
NONE, Y, XM, BITS = range(4)
ARGS = "dy mask_kind mask x gamma beta mean rstd dx dres dgamma dbeta accumulate workspace dtype rows C stream".split()
SCALARS = {"mask_kind", "accumulate", "dtype", "rows", "C", "stream"}
PTRS = [a for a in ARGS if a not in SCALARS]


def frozen_form_is_legal(kind, dtype, present):
    """the header's rules, spelled out: dy, rstd, dx always; gamma optional; the mask for MASK_Y / MASK_BITS; x and
    mean exactly when the mask is rebuilt from x or dgamma is wanted; beta (optional) under MASK_X only; dres optional
    without a mask or with MASK_Y, absent under MASK_X, required (bf16) under MASK_BITS; the workspace exactly when a
    parameter gradient is wanted"""
    p = set(present)
    if not {"dy", "rstd", "dx"} <= p:
        return False
    params = bool(p & {"dgamma", "dbeta"})
    reads_x = kind == XM or "dgamma" in p
    if ("x" in p) != reads_x or ("mean" in p) != reads_x or ("workspace" in p) != params:
        return False
    if ("mask" in p) != (kind in (Y, BITS)):
        return False
    if "beta" in p and kind != XM:
        return False
    if kind == XM and "dres" in p:
        return False
    if kind == BITS and ("dres" not in p or dtype != BF16):
        return False
    return True


def check_frozen_argument_validation():
    """every pointer subset x mask kind x dtype outside the table comes back as SSL4GIE_EARG -> (accepted, rejected)"""
    lib = _lib.load()
    rows, C = 4, 8
    nbytes = max(lib.ssl4gie_bn_workspace_bytes(rows, C), 4 * rows * C)
    bufs = {p: np.zeros(nbytes, dtype=np.uint8) for p in PTRS}

    def call(present, **scalars):
        vals = dict(mask_kind=NONE, accumulate=0, dtype=F32, rows=rows, C=C, stream=None)
        vals.update(scalars)
        return lib.ssl4gie_bn_bwd_frozen(*[(bufs[a].ctypes.data if a in present else None) if a in bufs else vals[a]
                                           for a in ARGS])
    accepted = rejected = 0
    legal = {}
    for kind, dtype in itertools.product(range(4), (F32, BF16)):
        for bits in itertools.product((0, 1), repeat=len(PTRS)):
            present = frozenset(itertools.compress(PTRS, bits))
            if frozen_form_is_legal(kind, dtype, present):
                accepted += 1
                legal.setdefault((kind, dtype), []).append(present)
                continue
            rc = call(present, mask_kind=kind, dtype=dtype)
            assert rc == EARG, (kind, dtype, sorted(present), rc)
            rejected += 1
    # the table itself (a typo shows up here): gamma free x {no gradient, dgamma, dbeta, both} = 8 everywhere; NONE / Y:
    # x dres free = 16 per dtype; X: x beta free = 16 per dtype; BITS: 8, bf16 only
    assert accepted == 2 * (16 + 16 + 16) + 8 and rejected > 100 * accepted, (accepted, rejected)
    # sizes, dtype codes and selectors no kernel serves, on forms that are otherwise legal
    for (kind, dtype), forms in legal.items():
        v = 8 if dtype == BF16 else 4
        bad = [{"C": 0}, {"C": -8}, {"C": v + v // 2}, {"C": 2}, {"rows": 0}, {"rows": -4}, {"dtype": 2}, {"dtype": -1},
               {"mask_kind": 4}, {"mask_kind": -1}]
        for present in (min(forms, key=len), max(forms, key=len)):
            for b in bad:
                rc = call(present, **dict(dict(mask_kind=kind, dtype=dtype), **b))
                assert rc == EARG, (kind, dtype, sorted(present), b, rc)
    return accepted, rejected


def test_every_illegal_pointer_combination_is_an_argument_error():
    check_frozen_argument_validation()


def test_the_addition_keeps_the_abi_version():
    assert _lib.load().ssl4gie_abi_version() == 13 == _lib.ABI_VERSION
