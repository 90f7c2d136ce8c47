"""The linear-probe pieces that need no GPU: the rank rule against torch.topk, the SGD / head restatements of
tests/probe_checks.py against torch and against the reference's recorded run (G22), the one-draw crop rule against its
Python loop, the probe helpers on CPU modules, and the torch fallbacks of the top-k metrics."""
import math

import numpy as np
import pytest
import torch
import torch.nn as nn

import probe_checks as pc
from conftest import load_golden, rel_err

CS = (5, 6, 63, 64, 65, 1000, 1003)
SIZES = pc.CROP_SIZES
crop_uniforms = pc.crop_uniforms   # the GPU test uploads the same uniforms


# ---------------------------------------------------------------------------------------------- rank rule
@pytest.mark.parametrize("C", CS)
def test_rank_rule_equals_topk_on_tie_free_rows(C):
    """rows that are permutations of C distinct values leave torch.topk no choice: hits at k = 1..5 must agree"""
    from ssl4gie_amd.metrics import topk_ranks_torch
    B = 33
    x = pc.permutation_rows(B, C, seed=C)
    g = torch.Generator().manual_seed(1000 + C)
    target = torch.randint(0, C, (B,), generator=g)
    target[0], target[1] = 0, C - 1
    _, pred = x.topk(5, 1, True, True)
    correct = pred.t().eq(target.view(1, -1).expand_as(pred.t()))
    rank = pc.ranks(x, target)
    rank_t, ok, _ = topk_ranks_torch(x, target)
    assert torch.equal(rank, rank_t) and bool(ok.all())
    for k in range(1, 6):
        assert int(correct[:k].reshape(-1).sum()) == int((rank < k).sum()), k


def test_rank_rule_on_ties_nans_and_rejected_rows():
    from ssl4gie_amd.metrics import topk_ranks_torch
    nan = float("nan")
    x = torch.tensor([[1.0, 1.0, 1.0, 1.0],      # all equal: rank = target
                      [0.0, nan, 2.0, nan],      # target 2: two NaNs above
                      [0.0, nan, 2.0, nan],      # target 3 (NaN): the NaN at 1 above
                      [0.0, nan, 2.0, nan],      # target 1 (NaN): nothing above
                      [3.0, 1.0, 3.0, 0.0],      # target 2: the equal value at 0 above
                      [1.0, 2.0, 3.0, 4.0],      # target -1: rejected
                      [1.0, 2.0, 3.0, 4.0]])     # target 4: rejected
    target = torch.tensor([2, 2, 3, 1, 2, -1, 4])
    want = torch.tensor([2, 2, 1, 0, 1, -1, -1])
    assert torch.equal(pc.ranks(x, target), want)
    rank, ok, loss = topk_ranks_torch(x, target)
    assert torch.equal(rank, want) and ok.tolist() == [True] * 5 + [False] * 2
    assert bool(loss[1:4].isnan().all()) and loss[5:].tolist() == [0.0, 0.0] and bool(torch.isfinite(loss[0]))
    ref = pc.row_losses(x, target)
    assert rel_err(loss[[0, 4]], ref[[0, 4]]) < 1e-6


# ---------------------------------------------------------------------------------------------- SGD, the head
@pytest.mark.parametrize("momentum,wd", [(0.0, 0.0), (0.9, 0.0), (0.9, 1e-2), (0.0, 1e-2)])
def test_sgd_restatement_equals_torch_sgd(momentum, wd):
    g = torch.Generator().manual_seed(3)
    p = torch.randn(64, 3, dtype=torch.float64, generator=g)
    grads = [torch.randn(64, 3, dtype=torch.float64, generator=g) for _ in range(3)]
    q = nn.Parameter(p.clone())
    opt = torch.optim.SGD([q], lr=0.1, momentum=momentum, weight_decay=wd)
    buf = torch.zeros_like(p)
    for gr in grads:
        q.grad = gr.clone()
        opt.step()
        p, buf = pc.sgd_step(p, gr, buf, 0.1, momentum, wd)
        assert rel_err(p, q.detach()) < 1e-14


def test_g22_curve_equals_the_head_restatement():
    """the reference's recorded fp64 run (its own LARS, torch's BatchNorm1d / Linear / CrossEntropyLoss) against
    probe_checks.probe_head_curve in fp64"""
    g = load_golden("g22_linprobe.npz")
    x, target = torch.from_numpy(g["x"]).double(), torch.from_numpy(g["target"])
    curve = pc.probe_head_curve(x, target, torch.from_numpy(g["weight0"]).double(),
                                torch.from_numpy(g["bias0"]).double(), float(g["lr"]), float(g["weight_decay"]),
                                float(g["momentum"]), float(g["trust_coefficient"]))
    for s, vals in enumerate(curve):
        for k, v in zip(("loss", "weight", "bias", "running_mean", "running_var"), vals):
            assert rel_err(v.reshape(g[f"fp64/{k}"][s].shape), g[f"fp64/{k}"][s]) < 1e-10, (s, k)
    moved = np.linalg.norm(g["fp64/weight"][-1] - g["weight0"]) / np.linalg.norm(g["weight0"])
    assert moved > 0.02, "the recorded run must move the weight far more than the 1e-3 bar it is held to"
    assert np.array_equal(g["x"], torch.from_numpy(g["x"]).bfloat16().float().numpy()), "x is bf16-representable"


# ---------------------------------------------------------------------------------------------- crop rule
@pytest.mark.parametrize("Hs,Ws", SIZES)
def test_tf_rrc_boxes_equals_the_python_loop(Hs, Ws):
    from ssl4gie_amd.data import tf_rrc_boxes
    u = crop_uniforms()
    want, margin = pc.tf_boxes(u, Hs, Ws)
    got = tf_rrc_boxes(u, Hs, Ws, (0.08, 1.0), (3.0 / 4.0, 4.0 / 3.0))
    assert got.dtype == torch.int32 and torch.equal(got, want)
    top, left, h, w = (got[:, i].long() for i in range(4))
    assert bool(((top >= 0) & (left >= 0) & (h >= 1) & (w >= 1) & (top + h <= Hs) & (left + w <= Ws)).all())
    # a 1-ulp difference in the fp32 exp moves a side of at most 256 by < 256 * 1.2e-7 / 2 = 1.6e-5: no rounding flips
    assert margin >= 5e-5, margin


def test_tf_rrc_boxes_smallest_side_and_clamp():
    from ssl4gie_amd.data import tf_rrc_boxes
    u = crop_uniforms()
    sides = [int(tf_rrc_boxes(u, Hs, Ws)[:, 2:].min()) for Hs, Ws in SIZES]
    assert min(sides) == 11, sides
    got = tf_rrc_boxes(u, 37, 53)
    over = [pc.tf_box(row, 37, 53, (0.08, 1.0), (3.0 / 4.0, 4.0 / 3.0))[1][1] > 37.5 for row in u.tolist()]
    assert any(over) and int(got[:, 2].max()) == 37, "a draw taller than the image is clamped to it"
    assert bool((got[torch.tensor(over), 2] == 37).all())


def test_random_resized_crop_flip_sampler_argument():
    from ssl4gie_amd.data import MAELinprobeTransform, RandomResizedCropFlip, rrc_boxes, tf_rrc_boxes
    with pytest.raises(ValueError):
        RandomResizedCropFlip(sampler="byol")
    assert RandomResizedCropFlip().sampler == "torchvision"
    t = MAELinprobeTransform(224, generator=torch.Generator().manual_seed(5))
    assert (t.sampler, t.scale, t.interpolation) == ("tf", (0.08, 1.0), "bicubic")
    box, flip = t.draw(64, 256, 256, "cpu")
    g = torch.Generator().manual_seed(5)
    u = torch.rand(64, 4, dtype=torch.float64, generator=g)
    assert torch.equal(box, tf_rrc_boxes(u, 256, 256, (0.08, 1.0)))
    # the default rule draws what it always drew
    d = RandomResizedCropFlip(generator=torch.Generator().manual_seed(6))
    box, _ = d.draw(8, 256, 256, "cpu")
    u = torch.rand(8, 10, 4, dtype=torch.float64, generator=torch.Generator().manual_seed(6))
    assert torch.equal(box, rrc_boxes(u, 256, 256))
    ev = MAELinprobeTransform.eval(224)
    assert (ev.stored, ev.offset) == (256, 16)


# ---------------------------------------------------------------------------------------------- probe helpers
def _tiny_vit(**kw):
    from ssl4gie_amd.Models.mae.models_vit import VisionTransformer
    return VisionTransformer(img_size=32, embed_dim=64, depth=1, num_heads=2, num_classes=10, **kw)


def test_mae_linear_probe_builds_the_reference_head():
    from ssl4gie_amd.probe import mae_linear_probe
    m = _tiny_vit()
    before = set(m.state_dict())
    w0 = m.head.weight.detach().clone()
    assert mae_linear_probe(m) is m
    keys = set(m.state_dict())
    assert keys - before == {"head.0.running_mean", "head.0.running_var", "head.0.num_batches_tracked",
                             "head.1.weight", "head.1.bias"}
    assert before - keys == {"head.weight", "head.bias"}
    bn = m.head[0]
    assert isinstance(bn, nn.BatchNorm1d) and not bn.affine and bn.eps == 1e-6 and bn.num_features == 64
    trainable = {n for n, p in m.named_parameters() if p.requires_grad}
    assert trainable == {"head.1.weight", "head.1.bias"}
    w = m.head[1].weight.detach()
    assert not torch.equal(w, w0) and 0.005 < float(w.std()) < 0.015   # trunc_normal_(std=0.01): cut at +-2, not +-2 std
    with pytest.raises(TypeError):
        mae_linear_probe(m)  # the head is no longer an nn.Linear


def test_vit_head_forms():
    m = _tiny_vit()
    m.head = nn.Sequential(nn.BatchNorm1d(64), nn.Linear(64, 10))   # affine BatchNorm: not the probe's head
    with pytest.raises(TypeError, match="BatchNorm1d"):
        m._head(torch.zeros(2, 64))
    m.head = nn.ReLU()
    with pytest.raises(TypeError):
        m._head(torch.zeros(2, 64))
    m.head = nn.Identity()
    assert m._head(torch.ones(2, 64, dtype=torch.bfloat16)).dtype == torch.float32


def _moco_checkpoint(model, linear_keyword):
    sd = {"module.base_encoder." + k: v.clone() for k, v in model.state_dict().items()}
    sd["module.base_encoder.%s.2.weight" % linear_keyword] = torch.zeros(3)   # the projector MoCo put in its place
    sd["module.momentum_encoder.cls_token"] = torch.zeros(1)
    sd["module.predictor.0.weight"] = torch.zeros(3)
    return sd


def test_moco_probe_helpers_and_sanity_check():
    from ssl4gie_amd.probe import adjust_learning_rate, load_moco_pretrained, moco_linear_probe, sanity_check
    src = _tiny_vit()
    ckpt = _moco_checkpoint(src, "head")
    m = _tiny_vit()
    assert moco_linear_probe(m, "head") is m
    assert {n for n, p in m.named_parameters() if p.requires_grad} == {"head.weight", "head.bias"}
    assert float(m.head.bias.detach().abs().max()) == 0.0 and 0.005 < float(m.head.weight.detach().std()) < 0.015
    n_before = len(ckpt)
    msg = load_moco_pretrained(m, ckpt, "head")
    assert set(msg.missing_keys) == {"head.weight", "head.bias"} and len(ckpt) == n_before
    assert torch.equal(m.blocks[0].attn.qkv.weight, src.blocks[0].attn.qkv.weight)
    with pytest.raises(AssertionError):
        load_moco_pretrained(_tiny_vit(), {k: v for k, v in ckpt.items() if "cls_token" not in k}, "head")
    sanity_check(m.state_dict(), ckpt, "head")
    with torch.no_grad():
        m.head.weight.add_(1.0)            # the linear layer may change
    sanity_check(m.state_dict(), ckpt, "head")
    with torch.no_grad():
        m.blocks[0].mlp.fc1.bias[3] += 1e-3
    with pytest.raises(AssertionError, match="blocks.0.mlp.fc1.bias is changed"):
        sanity_check(m.state_dict(), ckpt, "head")
    sanity_check({"module." + k: v for k, v in src.state_dict().items()}, ckpt, "head")   # a DDP-wrapped model's keys

    class Opt:
        param_groups = [{"lr": 0.0}, {"lr": 0.0}]
    assert adjust_learning_rate(Opt, 0.1, 0, 90) == 0.1
    assert abs(adjust_learning_rate(Opt, 0.1, 45, 90) - 0.05) < 1e-12 and Opt.param_groups[1]["lr"] == 0.05


def test_resnet_probe_helpers_and_sanity_check_on_running_statistics():
    from ssl4gie_amd.Models.resnet import resnet50
    from ssl4gie_amd.probe import load_moco_pretrained, moco_linear_probe, sanity_check
    src = resnet50(num_classes=7)
    ckpt = _moco_checkpoint(src, "fc")
    m = moco_linear_probe(resnet50(num_classes=7), "fc")
    assert {n for n, p in m.named_parameters() if p.requires_grad} == {"fc.weight", "fc.bias"}
    load_moco_pretrained(m, ckpt, "fc")
    sanity_check(m.state_dict(), ckpt, "fc")
    with torch.no_grad():
        m.layer3[2].bn2.running_var[5] *= 1.001   # "e.g., BN stats updated"
    with pytest.raises(AssertionError, match="layer3.2.bn2.running_var is changed"):
        sanity_check(m.state_dict(), ckpt, "fc")
    from ssl4gie_amd.Models.resnet import ResNet50
    with pytest.raises(RuntimeError, match="fc"):
        ResNet50().forward(torch.zeros(1, 3, 64, 64))


def test_arena_sgd_and_lars_signatures():
    from ssl4gie_amd.Models.mae.util.lars import LARS
    from ssl4gie_amd.optim import ArenaSGD
    m = _tiny_vit()
    with pytest.raises(NotImplementedError):
        ArenaSGD(m, m.head.parameters(), 0.1, nesterov=True, momentum=0.9)
    with pytest.raises(NotImplementedError):
        ArenaSGD(m, m.head.parameters(), 0.1, dampening=0.1)
    opt = LARS(m.head.parameters(), lr=0.3)
    assert opt.param_groups[0]["lr"] == 0.3 and opt.param_groups[0]["weight_decay"] == 0
    assert (opt.param_groups[0]["momentum"], opt.param_groups[0]["trust_coefficient"]) == (0.9, 0.001)
    opt.param_groups[0]["lr"] = 0.1      # lr_sched.adjust_learning_rate writes here
    sd = opt.state_dict()
    assert sd["kind"] == "LARS" and sd["state"] == {"mu": None} and sd["param_groups"][0]["lr"] == 0.1
    opt.load_state_dict(sd)
    with pytest.raises(RuntimeError, match="arena"):
        opt.step()                        # CPU parameters live in no engine arena


# ---------------------------------------------------------------------------------------------- metrics fallbacks
def _metric_case():
    x = pc.permutation_rows(40, 23, seed=7)
    x[3] = 1.0                       # an all-equal row
    x[5, 2] = float("nan")
    g = torch.Generator().manual_seed(8)
    target = torch.randint(0, 23, (40,), generator=g)
    target[7], target[9] = -1, 23
    return x, target


def test_topk_accuracy_torch_fallback():
    from ssl4gie_amd.metrics import TopKAccuracy
    x, target = _metric_case()
    m = TopKAccuracy((1, 5))
    assert m.compute()["n"] == 0 and math.isnan(m.compute()["acc1"])
    m.update(x[:16], target[:16])
    m.update(x[16:].bfloat16().float(), target[16:])
    # the second part was rounded to bf16: score the restatement on the same numbers
    xr = torch.cat([x[:16], x[16:].bfloat16().float()])
    rank = pc.ranks(xr, target)
    want = pc.topk_counts(rank, (1, 5))
    loss = pc.row_losses(xr, target)
    out = m.compute()
    assert set(out) == {"acc1", "acc5", "loss", "n", "rejected"}
    assert (out["n"], out["rejected"]) == (want[2], want[3]) == (38, 2)
    assert out["acc1"] == 100.0 * want[0] / want[2] and out["acc5"] == 100.0 * want[1] / want[2]
    assert math.isnan(out["loss"]) and math.isnan(float(loss.sum()))   # the NaN row reaches the sum
    m.reset()
    keep = torch.arange(40) != 5
    m.update(x[keep], target[keep])
    out = m.compute()
    ref = pc.row_losses(x[keep], target[keep])
    assert abs(out["loss"] - float(ref.sum()) / out["n"]) < 1e-6 * abs(float(ref.sum()) / out["n"])
    with pytest.raises(ValueError):
        TopKAccuracy((1, 5)).update(x[:, :4], target)       # k > C
    with pytest.raises(ValueError):
        TopKAccuracy((5, 1))


def test_accuracy_torch_fallback_equals_the_drivers_formulation():
    from ssl4gie_amd.metrics import accuracy
    x = pc.permutation_rows(64, 100, seed=9)
    target = torch.randint(0, 100, (64,), generator=torch.Generator().manual_seed(10))
    _, pred = x.topk(5, 1, True, True)
    correct = pred.t().eq(target.view(1, -1).expand_as(pred.t()))
    want = [correct[:k].reshape(-1).float().sum(0, keepdim=True).mul_(100.0 / 64) for k in (1, 5)]
    got = accuracy(x, target, topk=(1, 5))
    assert [tuple(t.shape) for t in got] == [(1,), (1,)] and got[0].dtype == torch.float32
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    assert torch.equal(accuracy(x, target)[0], want[0])
    with pytest.raises(ValueError):
        accuracy(x[:, :3], target, topk=(1, 5))
