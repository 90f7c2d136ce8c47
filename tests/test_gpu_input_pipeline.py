"""GPU: the on-device input pipeline — ssl4gie_view_sample_u8 against the fp64 restatement of its resampling rule
(tests/input_checks.py), its guards and repeatability, and ssl4gie_amd.data feeding the MAE statement sequence.

Bar of the parity tests: 4 x the error of torch's own CPU fp32 F.interpolate(antialias=True) on the same cases, per
filter, computed here (input_checks.torch_cpu_error) — the kernel sums in another order (row pass first, through an
fp32 LDS tile) and rounds its weights to fp32."""
import math
import types

import numpy as np
import pytest
import torch

import input_checks as ic

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
U255 = dict(mean=(0.0, 0.0, 0.0), std=(1.0 / 255.0,) * 3)   # output in 0..255 units


@pytest.fixture(scope="module")
def bank():
    """n = 3 images of 96 x 81 (243-byte rows) — the first 3 of a 5-image allocation, so that an index or box the
    kernel failed to refuse would read finite values inside the allocation rather than fault.  Image 1 is the
    noise image of the fixed cases."""
    from ssl4gie_amd import _lib
    _lib.load()
    imgs = np.stack([ic.noise_image(s) for s in (7, 0, 9, 11, 12)])
    whole = torch.from_numpy(imgs).to(DEV)
    return types.SimpleNamespace(np=imgs[:3], dev=whole[:3], whole=whole)


def _boxes(rows):
    return torch.tensor(rows, dtype=torch.int32, device=DEV)


def _run(bank, index, boxes, flips, S, name, **kw):
    from ssl4gie_amd import ops
    idx = torch.tensor(index, dtype=torch.int64, device=DEV)
    fl = None if flips is None else torch.tensor(flips, dtype=torch.uint8, device=DEV)
    return ops.view_sample_u8(bank.dev, idx, _boxes(boxes), fl, S, name, **kw)


@pytest.mark.parametrize("name", ic.FILTERS)
def test_view_sample_matches_fp64_restatement_on_the_fixed_cases(bank, name):
    bar = 4.0 * ic.torch_cpu_error()[name]
    worst = 0.0
    for S in ic.SIZES:
        boxes = [b for b in ic.BOXES for _ in (0, 1)]
        flips = [f for _ in ic.BOXES for f in (0, 1)]
        got = _run(bank, [1] * len(boxes), boxes, flips, S, name, **U255).cpu().numpy().astype(np.float64)
        assert got.shape == (len(boxes), 3, S, S)
        for k, (box, f) in enumerate(zip(boxes, flips)):
            worst = max(worst, float(np.abs(got[k] - ic.view_ref(bank.np[1], box, S, name, bool(f))).max()))
    print(f"view_sample_u8 {name}: max |kernel - fp64| = {worst:.3e} (0..255 units), bar {bar:.3e}")
    assert worst <= bar, (name, worst, bar)


def test_view_sample_imagenet_constants_and_mixed_indices(bank):
    from ssl4gie_amd.ops import IMAGENET_MEAN, IMAGENET_STD
    index = [2, 0, 1, 0, 2, 1]
    boxes = [ic.BOXES[k] for k in (4, 1, 5, 0, 2, 3)]
    flips = [1, 0, 0, 1, 0, 1]
    for name in ic.FILTERS:
        got = _run(bank, index, boxes, flips, 24, name).cpu().numpy().astype(np.float64)   # ImageNet mean / std
        bar = 4.0 * ic.torch_cpu_error()[name] / (255.0 * 0.224)
        for k in range(len(index)):
            ref = ic.view_ref(bank.np[index[k]], boxes[k], 24, name, bool(flips[k]), IMAGENET_MEAN, IMAGENET_STD)
            err = float(np.abs(got[k] - ref).max())
            assert err <= bar, (name, k, err, bar)


def test_view_sample_production_tile_upsampling(bank):
    """B = 2, S = 224, whole-image box of 96 x 81: several bands per sample, up-sampling on both axes"""
    box = (0, 0, ic.H_IMG, ic.W_IMG)
    for name in ic.FILTERS:
        got = _run(bank, [1, 2], [box, box], [0, 1], 224, name, **U255).cpu().numpy().astype(np.float64)
        bar = 4.0 * ic.torch_cpu_error()[name]
        for k, (i, f) in enumerate(((1, False), (2, True))):
            err = float(np.abs(got[k] - ic.view_ref(bank.np[i], box, 224, name, f)).max())
            print(f"view_sample_u8 {name} S=224 whole image: {err:.3e}, bar {bar:.3e}")
            assert err <= bar, (name, k, err, bar)


def test_view_sample_guards(bank):
    from ssl4gie_amd import ops
    good = (5, 7, 17, 23)
    Hs, Ws = ic.H_IMG, ic.W_IMG
    bad = [(3, good), (-1, good), (1, (Hs + 3 - 20, 0, 20, 10)), (1, (0, 0, 10, 0)), (1, (0, -1, 10, 10)),
           (1, (0, 0, 0, 10)), (1, (-2, 0, 10, 10)), (1, (0, Ws - 9, 10, 10))]
    index = [1, 2] + [i for i, _ in bad] + [0]
    boxes = [good, ic.BOXES[4]] + [b for _, b in bad] + [ic.BOXES[2]]
    flips = [0, 1] + [1, 0] * (len(bad) // 2) + [1]
    for name in ic.FILTERS:
        out = _run(bank, index, boxes, flips, 24, name)
        clean = _run(bank, [1, 2, 0], [good, ic.BOXES[4], ic.BOXES[2]], [0, 1, 1], 24, name)
        for k in range(len(bad)):
            assert bool(torch.isnan(out[2 + k]).all()), (name, bad[k])
        # the neighbours of the refused samples are bit-identical to a batch without them
        assert torch.equal(out[0], clean[0]) and torch.equal(out[1], clean[1]) and torch.equal(out[-1], clean[2])
        assert bool(torch.isfinite(clean).all())
    idx = torch.tensor([1], dtype=torch.int64, device=DEV)
    for kw in (dict(S=30), dict(S=24, std=(0.229, 0.0, 0.225)), dict(S=24, filter=7)):
        S = kw.pop("S")
        with pytest.raises(RuntimeError, match="invalid argument"):
            ops.view_sample_u8(bank.dev, idx, _boxes([good]), None, S, **kw)
    torch.cuda.synchronize()


def test_view_sample_is_repeatable_and_flip_none_is_no_flip(bank):
    n = len(ic.BOXES)
    index = [k % 3 for k in range(n)]
    for name in ic.FILTERS:
        a = _run(bank, index, list(ic.BOXES), [k % 2 for k in range(n)], 32, name)
        b = _run(bank, index, list(ic.BOXES), [k % 2 for k in range(n)], 32, name)
        assert torch.equal(a, b)
        assert torch.equal(_run(bank, index, list(ic.BOXES), None, 32, name),
                           _run(bank, index, list(ic.BOXES), [0] * n, 32, name))
        assert torch.equal(a[1], _run(bank, index, list(ic.BOXES), [0] * n, 32, name)[1].flip(-1))


def test_device_loader_feeds_the_mae_statement_sequence():
    """engine_pretrain.py:39-57 as written, over a DeviceLoader on a 16-image bank; and the batch the loader yields
    is ops.view_sample_u8 on the boxes its transform's generator seed gives"""
    from ssl4gie_amd import ops
    from ssl4gie_amd.data import DeviceImageBank, DeviceLoader, RandomResizedCropFlip
    from ssl4gie_amd.Models.mae import models_mae
    from ssl4gie_amd.Models.mae.util import lr_sched, misc
    device = torch.device(DEV)
    imgs = np.stack([ic.noise_image(100 + s, 48, 40) for s in range(16)])
    bank = DeviceImageBank.from_uint8(imgs, device, labels=np.arange(16) % 4)

    def make_loader(seed):
        tf = RandomResizedCropFlip(32, scale=(0.2, 1.0), generator=torch.Generator(device=device).manual_seed(seed))
        return DeviceLoader(bank, 8, sampler=torch.utils.data.SequentialSampler(bank), transform=tf)

    # the loader's batch == the kernel on the same draw
    samples, labels = next(iter(make_loader(11)))
    twin = RandomResizedCropFlip(32, scale=(0.2, 1.0), generator=torch.Generator(device=device).manual_seed(11))
    box, flip = twin.draw(8, 48, 40, device)
    index = torch.arange(8, device=device)
    assert samples.shape == (8, 3, 32, 32) and samples.dtype == torch.float32 and samples.device == device
    assert torch.equal(samples, ops.view_sample_u8(bank.images, index, box, flip, 32, "bicubic"))
    assert torch.equal(labels.cpu(), torch.arange(8) % 4)
    top, left, h, w = box.cpu().unbind(1)
    assert bool(((h >= 1) & (w >= 1) & (top >= 0) & (left >= 0) & (top + h <= 48) & (left + w <= 40)).all())
    k = 3
    ref = ic.view_ref(imgs[k], tuple(int(v) for v in box[k].cpu()), 32, "bicubic", bool(flip[k]), ops.IMAGENET_MEAN,
                      ops.IMAGENET_STD)
    assert float(np.abs(samples[k].cpu().numpy() - ref).max()) <= 4.0 * ic.torch_cpu_error()["bicubic"] / (255.0 * 0.224)
    two = RandomResizedCropFlip(32, interpolation="bilinear", views=2,
                                generator=torch.Generator(device=device).manual_seed(5))(bank, index)
    assert isinstance(two, list) and len(two) == 2 and not torch.equal(two[0], two[1])

    # three steps of the reference's loop
    torch.manual_seed(0)
    model = models_mae.MaskedAutoencoderViT(img_size=32, patch_size=16, embed_dim=64, depth=2, num_heads=2,
                                            decoder_embed_dim=64, decoder_depth=1, decoder_num_heads=2,
                                            mlp_ratio=4).to(device).set_precision("bf16")
    optimizer = torch.optim.AdamW(model.parameters(), lr=1e-3, betas=(0.9, 0.95))
    loss_scaler = misc.NativeScalerWithGradNormCount()
    args = types.SimpleNamespace(accum_iter=1, mask_ratio=0.75, lr=1e-3, min_lr=0.0, warmup_epochs=1, epochs=2)
    data_loader = make_loader(12)
    assert len(data_loader) == 2
    accum_iter = args.accum_iter
    losses = []
    optimizer.zero_grad()
    for epoch in range(2):
        for data_iter_step, (samples, _) in enumerate(data_loader):
            if len(losses) == 3:
                break
            if data_iter_step % accum_iter == 0:
                lr_sched.adjust_learning_rate(optimizer, data_iter_step / len(data_loader) + epoch, args)
            samples = samples.to(device, non_blocking=True)
            with torch.cuda.amp.autocast():
                loss, _, _ = model(samples, mask_ratio=args.mask_ratio)
            loss_value = loss.item()
            assert math.isfinite(loss_value), loss_value
            loss /= accum_iter
            loss_scaler(loss, optimizer, parameters=model.parameters(),
                        update_grad=(data_iter_step + 1) % accum_iter == 0)
            if (data_iter_step + 1) % accum_iter == 0:
                optimizer.zero_grad()
            torch.cuda.synchronize()
            losses.append(loss_value)
    assert len(losses) == 3 and all(math.isfinite(v) for v in losses)


def test_view_sample_largest_supported_stored_size():
    """Hs = Ws = 1024 -> S = 224, whole-image box: 19 taps per axis, and an LDS plan beyond 64 KiB (the band shrinks
    to fit the whole-image box into the CU's LDS).  Bar: 4 x torch's CPU fp32 error on this very case."""
    from ssl4gie_amd import ops
    img = ic.noise_image(21, 1024, 1024)
    box = (0, 0, 1024, 1024)
    dev = torch.from_numpy(img[None]).to(DEV)
    idx = torch.zeros(1, dtype=torch.int64, device=DEV)
    for name in ic.FILTERS:
        got = ops.view_sample_u8(dev, idx, _boxes([box]), None, 224, name, **U255).cpu().numpy().astype(np.float64)
        ref = ic.view_ref(img, box, 224, name)
        bar = 4.0 * float(np.abs(ic.torch_cpu_view(img, box, 224, name).astype(np.float64) - ref).max())
        err = float(np.abs(got[0] - ref).max())
        print(f"view_sample_u8 {name} 1024^2 whole image: {err:.3e}, bar {bar:.3e}")
        assert err <= bar, (name, err, bar)
