"""GPU: ssl4gie_amd.Models.deeplab.DeepLabV3Plus against the fp64 restatement of smp 0.3.2's model (tests/deeplab_checks.py,
unpinned: smp is installed nowhere), same weights, Dropout.p = 0 on both sides.

Inputs are [4, 3, 64, 64]: the layer4 map is 4 x 4 and the rates 12 / 24 / 36 reduce to the centre tap; the non-square
[2, 3, 96, 128] case runs in eval mode (with two images the pooling branch's BatchNorm sees two rows, whose
normalised values are +-1 whatever the data: no training-mode gradient through it is well conditioned).

CONDITION on the training inputs, checked here on the CPU: the restatement in fp32 agrees with itself in fp64 to
<= 1e-4 per tensor (conftest.rel_err) on the logits, every parameter gradient and every running statistic.  A ReLU
network's gradient is discontinuous where a pre-activation crosses zero, and on 4 x 4 maps a single crossing moves a
weight gradient by percents; deeplab_checks.model_inputs / model_weights were chosen (seed, weak residual branches) so
that fp32 rounding crosses none: with gamma ~ 1 on every bn3 and i.i.d. noise images the restatement's own fp32
gradients are 2e-2 off its fp64 ones.
"""
import numpy as np
import pytest
import torch

import deeplab_checks as chk
from conftest import rel_err

pytestmark = pytest.mark.gpu
DEV = "cuda"
SHAPE = (4, 3, 64, 64)


def _engine_model(sd, prec, train=True):
    from ssl4gie_amd.Models.deeplab import DeepLabV3Plus
    m = DeepLabV3Plus("resnet50", encoder_weights=None, classes=1)
    m.load_state_dict(sd)
    m.decoder.aspp[0].project[3].p = 0.0
    m.to(DEV).set_precision(prec)
    return m.train() if train else m.eval()


def _engine_step(prec):
    from ssl4gie_amd.resnet_engine import flush_batch_counts
    r = chk.reference(SHAPE)
    m = _engine_model(r["sd"], prec)
    out = m(r["imgs"].to(DEV))
    assert out.shape == (SHAPE[0], 1, *SHAPE[2:]) and out.dtype == torch.float32
    (out * r["wy"].to(DEV)).sum().backward()
    torch.cuda.synchronize()
    flush_batch_counts(m)
    return r, m, out.detach()


def test_inputs_are_well_conditioned():
    """the condition of the module docstring (CPU arithmetic only: the engine is not involved)"""
    r = chk.reference(SHAPE)
    (o64, g64, s64), (o32, g32, s32) = r["f64"], r["f32"]
    worst = max([rel_err(o32, o64)] + [rel_err(g32[k], g64[k]) for k in g64] + [rel_err(s32[k], s64[k]) for k in s64])
    print(f"restatement fp32 against fp64, worst tensor: {worst:.3e}")
    assert worst <= 1e-4


def test_deeplab_fp32_parity():
    """logits, every parameter gradient and the running statistics after one step at the project's 1e-3"""
    r, m, out = _engine_step("fp32")
    o64, g64, s64 = r["f64"]
    errs = {"logits": rel_err(out, o64)}
    params = dict(m.named_parameters())
    assert set(params) == set(g64)
    for k, p in params.items():
        assert p.grad is not None, k
        errs[k] = rel_err(p.grad, g64[k])
    bufs = dict(m.named_buffers())
    for k in s64:
        errs[k] = rel_err(bufs[k], s64[k])
    worst = sorted(errs.items(), key=lambda kv: -kv[1])[:5]
    print("fp32 parity, worst tensors: " + ", ".join(f"{k} {v:.2e}" for k, v in worst))
    assert worst[0][1] < 1e-3, worst
    assert int(m.encoder.bn1.num_batches_tracked) == 1 and int(m.decoder.block2[1].num_batches_tracked) == 1


def _l2(a, b):
    a, b = a.detach().double().cpu(), b.double()
    return float((a - b).norm() / (b.norm() + 1e-300))


def test_deeplab_bf16_per_tensor():
    """G17's form (tests/test_gpu_models_golden.py:_bf16_gate): per-tensor relative L2 error of the bf16 engine against
    fp64, held to 1.5 x the distribution of the restatement's own error under torch.autocast("cpu", torch.bfloat16)
    on the same weights and inputs — median, 90th percentile, the worst well-sampled tensor (>= 1024 elements), and
    3 x the worst for the tiny ones; the logits to 1.5 x theirs.  The bars are computed here, not fixed."""
    r, m, out = _engine_step("bf16")
    o64, g64, _ = r["f64"]
    ob, gb, _ = r["bf16"]
    names = sorted(g64)
    params = dict(m.named_parameters())
    ref_err = np.array([_l2(gb[k], g64[k]) for k in names])
    errs = np.array([_l2(params[k].grad, g64[k]) for k in names])
    big = np.array([g64[k].numel() >= 1024 for k in names])
    e_out, r_out = _l2(out, o64), _l2(ob, o64)
    order = np.argsort(-errs)[:4]
    print(f"bf16 logits {e_out:.3e} (restatement under autocast {r_out:.3e}); gradients median {np.median(errs):.3e} "
          f"(ref {np.median(ref_err):.3e}), q90 {np.quantile(errs, 0.9):.3e} (ref {np.quantile(ref_err, 0.9):.3e}); worst "
          + ", ".join(f"{names[i]} {errs[i]:.3e} (ref {ref_err[i]:.3e})" for i in order))
    assert e_out <= 1.5 * r_out
    assert np.median(errs) <= 1.5 * np.median(ref_err)
    assert np.quantile(errs, 0.9) <= 1.5 * np.quantile(ref_err, 0.9)
    wb = int(np.argmax(np.where(big, errs, 0)))
    assert errs[wb] <= 1.5 * ref_err[big].max(), (names[wb], errs[wb], ref_err[big].max())
    assert errs.max() <= 3.0 * ref_err.max(), (names[int(errs.argmax())], errs.max(), ref_err.max())


@pytest.mark.parametrize("shape", [SHAPE, (2, 3, 96, 128)])
def test_deeplab_eval_no_grad(shape):
    """eval(): running statistics, no Dropout; logits in fp32 mode at 1e-3, on the square and the non-square input"""
    r = chk.reference(shape, training=False)
    m = _engine_model(r["sd"], "fp32", train=False)
    with torch.no_grad():
        out = m(r["imgs"].to(DEV))
    assert out.shape == (shape[0], 1, *shape[2:])
    e, e32 = rel_err(out, r["f64"][0]), rel_err(r["f32"][0], r["f64"][0])
    print(f"eval logits {shape}: {e:.3e} (restatement fp32 against fp64: {e32:.3e})")
    assert e32 <= 1e-4 and e < 1e-3
    for k, v in m.state_dict().items():   # eval mode leaves every buffer alone
        if k.endswith(("running_mean", "running_var")):
            assert torch.equal(v.cpu(), r["sd"][k]), k


def test_deeplab_three_classes_upsampling_two():
    """classes = 3 (the head's NCHW transposition, 3 of 8 padded GEMM columns) and upsampling = 2 (another integer scale):
    eval logits in fp32 mode at 1e-3; one training step gives every head and decoder parameter a finite gradient; the
    head's three gradients against fp64 autograd at 1e-3"""
    from ssl4gie_amd.Models.deeplab import DeepLabV3Plus
    sd = chk.model_weights(classes=3, upsampling=2)
    imgs, _ = chk.model_inputs((2, 3, 64, 64))
    flt = {k: (v.double() if v.is_floating_point() else v) for k, v in sd.items()}
    with torch.no_grad():
        want = chk.deeplab(flt, imgs.double(), training=False, upsampling=2)
    m = DeepLabV3Plus("resnet50", encoder_weights=None, classes=3, upsampling=2)
    m.load_state_dict(sd)
    m.to(DEV).set_precision("fp32").eval()
    with torch.no_grad():
        out = m(imgs.to(DEV))
    assert out.shape == (2, 3, 32, 32) and out.dtype == torch.float32 and out.is_contiguous()
    assert rel_err(out, want) < 1e-3
    m.train()
    wy = torch.randn(2, 3, 32, 32, generator=torch.Generator().manual_seed(1)).to(DEV)
    (m(imgs.to(DEV)) * wy).sum().backward()
    for k, p_ in m.named_parameters():
        if not k.startswith("encoder."):
            assert p_.grad is not None and bool(torch.isfinite(p_.grad).all()) and float(p_.grad.abs().max()) > 0, k
    # the head alone (linear, so well conditioned): SegHeadACFn on the engine's own decoder output against torch's
    # autograd through the 1x1 convolution and the up-sampling in fp64
    import torch.nn.functional as F
    from ssl4gie_amd.atrous_engine import SegHeadACFn
    h = m.segmentation_head[0]
    m.zero_grad()
    m._prepare()
    y = m.decode(*m.encoder.features(imgs.to(DEV))).detach().clone().requires_grad_(True)
    (SegHeadACFn.apply(y, h.weight, h.bias, 2, m.sink(), m.lp_cache) * wy).sum().backward()
    y64 = y.detach().double().cpu().permute(0, 3, 1, 2).requires_grad_(True)
    w64, b64 = h.weight.detach().double().cpu().requires_grad_(True), h.bias.detach().double().cpu().requires_grad_(True)
    ref = F.interpolate(F.conv2d(y64, w64, b64), scale_factor=2, mode="bilinear", align_corners=True)
    (ref * wy.double().cpu()).sum().backward()
    assert rel_err(y.grad.permute(0, 3, 1, 2), y64.grad) < 1e-3
    assert rel_err(h.weight.grad, w64.grad) < 1e-3 and rel_err(h.bias.grad, b64.grad) < 1e-3


def test_reference_training_loop_statements():
    """Binary_segmentation/train_segmentation.py:38-52 (train_epoch) with :204-205,254 (AdamW, GradScaler, SoftDiceLoss),
    the statements as written, on DeviceLoader + FinetuneAugment.segmentation() batches with ArenaAdamW: 20 steps on one
    fixed batch bring the loss below the first step's"""
    import torch.distributed as dist
    from ssl4gie_amd.data import DeviceImageBank, DeviceLoader, FinetuneAugment
    from ssl4gie_amd.losses import SoftDiceLoss
    from ssl4gie_amd.Models.deeplab import DeepLabV3Plus
    from ssl4gie_amd.optim import ArenaAdamW
    rank, world_size, S, B = 0, 1, 64, 4
    own_group = not dist.is_initialized()
    if own_group:
        import tempfile
        store = tempfile.NamedTemporaryFile(delete=False)
        dist.init_process_group("gloo", init_method=f"file://{store.name}", rank=0, world_size=1)
    try:
        torch.manual_seed(3)
        rng = np.random.default_rng(5)
        yy, xx = np.mgrid[0:S, 0:S]
        imgs, masks = np.empty((8, S, S, 3), np.uint8), np.empty((8, S, S), np.uint8)
        for i in range(8):   # a bright disc on noise, and its mask
            disc = (yy - rng.integers(16, 48)) ** 2 + (xx - rng.integers(16, 48)) ** 2 < rng.integers(8, 20) ** 2
            imgs[i] = np.clip(rng.normal(90, 30, (S, S, 3)) + 120 * disc[..., None], 0, 255).astype(np.uint8)
            masks[i] = 255 * disc
        bank = DeviceImageBank.from_uint8(imgs, torch.device(DEV), targets=masks)
        gen = torch.Generator(device=DEV).manual_seed(9)
        loader = DeviceLoader(bank, B, sampler=torch.utils.data.SequentialSampler(bank),
                              transform=FinetuneAugment.segmentation(S, generator=gen))
        train_loader = [next(iter(loader))] * 20   # one fixed batch
        model = DeepLabV3Plus("resnet50", encoder_weights=None, classes=1)
        model.cuda(rank).set_precision("bf16")
        optimizer = ArenaAdamW(model, list(model.parameters()), lr=1e-3)
        scaler = torch.cuda.amp.GradScaler()
        loss_fn = SoftDiceLoss()
        # ---- train_epoch, as written
        model.train()
        loss_accumulator = []
        for batch_idx, (data, target) in enumerate(train_loader):
            data, target = data.cuda(rank), target.cuda(rank)
            optimizer.zero_grad()
            with torch.cuda.amp.autocast():
                output = model(data)
                loss = loss_fn(output, target)
            scaler.scale(loss).backward()
            scaler.step(optimizer)
            scaler.update()
            dist.all_reduce(loss)
            loss /= world_size
            loss_accumulator.append(loss.item())
        # ----
    finally:
        if own_group:
            dist.destroy_process_group()
    print("loss, steps 1 / 10 / 20:", loss_accumulator[0], loss_accumulator[9], loss_accumulator[-1])
    assert all(np.isfinite(loss_accumulator)) and output.shape == (B, 1, S, S)
    assert loss_accumulator[-1] < loss_accumulator[0]
