"""CPU: the public loss heads of ssl4gie_amd.losses run the torch formulation on CPU tensors (bit-equal to
nn.CrossEntropyLoss; the reference's own InfoNCE fixture G8), and the C ABI declares and binds the fused entry points."""
import os
import re

import torch
import torch.nn as nn

from conftest import ROOT, load_golden, rel_err

NEW_SYMBOLS = ("ssl4gie_infonce_workspace_bytes", "ssl4gie_infonce_loss", "ssl4gie_cross_entropy_workspace_bytes",
               "ssl4gie_cross_entropy", "ssl4gie_bt_loss_workspace_bytes", "ssl4gie_bt_loss", "ssl4gie_bt_loss_grad")


def test_cross_entropy_on_cpu_tensors_is_torch_bit_for_bit():
    from ssl4gie_amd.losses import CrossEntropyLoss
    g = torch.Generator().manual_seed(0)
    for B, C in ((7, 6), (64, 12), (3, 1)):
        x = torch.randn(B, C, generator=g)
        t = torch.randint(0, C, (B,), generator=g)
        w = torch.rand(C, generator=g) + 0.1
        for weight in (None, w):
            fn = CrossEntropyLoss(weight)
            assert ("weight" in dict(fn.named_buffers())) == (weight is not None)
            a = x.clone().requires_grad_(True)
            b = x.clone().requires_grad_(True)
            la, lb = fn(a, t), nn.CrossEntropyLoss(weight)(b, t)
            la.backward()
            lb.backward()
            assert torch.equal(la, lb) and torch.equal(a.grad, b.grad)
    x4, t4 = torch.randn(2, 5, 3, 3, generator=g), torch.randint(0, 5, (2, 3, 3), generator=g)
    assert torch.equal(CrossEntropyLoss()(x4, t4), nn.CrossEntropyLoss()(x4, t4))


def test_info_nce_on_cpu_tensors_matches_reference_fixture():
    from ssl4gie_amd.losses import info_nce
    g = load_golden("g8_moco.npz")
    q = torch.from_numpy(g["cl/q"]).requires_grad_(True)
    loss = info_nce(q, torch.from_numpy(g["cl/k"]), float(g["cl/T"]), 0)
    loss.backward()
    assert abs(float(loss.detach()) - float(g["cl/loss"])) < 1e-6 * abs(float(g["cl/loss"]))
    assert rel_err(q.grad, g["cl/dq"]) < 1e-6


def test_header_declares_and_lib_binds_the_loss_head_symbols():
    from ssl4gie_amd import _lib
    txt = open(os.path.join(ROOT, "include", "ssl4gie_hip.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    declared = set(re.findall(r"\b(ssl4gie_[a-z0-9_]+)\s*\(", txt))
    for name in NEW_SYMBOLS:
        assert name in declared, name
        assert name in _lib.PROTOTYPES, name
    assert _lib.ABI_VERSION == 13
    L = _lib.load()
    assert L.ssl4gie_abi_version() == 13
    # workspace queries need no GPU
    assert L.ssl4gie_infonce_workspace_bytes(256, 2048, 256) > (256 + 2048) * 256 * 4
    assert L.ssl4gie_infonce_workspace_bytes(0, 8, 8) == 0
    assert L.ssl4gie_cross_entropy_workspace_bytes(256, 12) >= 256 * 4
    assert L.ssl4gie_bt_loss_workspace_bytes(8192) > 0 and L.ssl4gie_bt_loss_workspace_bytes(0) == 0
