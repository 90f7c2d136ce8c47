"""GPU: ssl4gie_color_augment_ft and ssl4gie_paired_warp against the restatements of their rules (tests/warp_checks.py,
pinned on the CPU by tests/test_warp_checks_cpu.py), their exactness properties and guards, and FinetuneAugment
through the DeviceLoader.

Colour stage: the bar is 4 x the largest error of the restatement's own float32 CPU evaluation against its float64
evaluation on the very same rows, computed here and printed — test_gpu_color_augment.py's bar.  Solarize is never
set (the finetune loaders have none), so nothing is masked.
Warp: a gather, so compared pixels are bit-equal; pixels whose float64 source coordinate lies within 1e-3 of a
half-integer (warp_checks.TIE_GUARD) may land on either neighbour and are not compared; they are at most 2 % of a
sample at S = 224 and 4 % at S = 16, 32."""
import ctypes as C

import numpy as np
import pytest
import torch

import colour_checks as cc
import warp_checks as wc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FILL = (-1.0, -0.5, 0.25)


@pytest.fixture(scope="module", autouse=True)
def _lib_loaded():
    from ssl4gie_amd import _lib
    _lib.load()


def _ft(rows, mean=cc.ZERO3, std=cc.ONE3):
    from ssl4gie_amd import ops
    return ops.color_augment_ft(*(t.to(DEV) for t in rows), mean, std)


def _hold(name, rows, ref64, err32, scale=1.0, mean=cc.ZERO3, std=cc.ONE3):
    got = _ft(rows, mean, std).cpu().to(torch.float64)
    assert got.shape == ref64.shape and bool(torch.isfinite(got).all())
    d = (got - ref64).abs()
    err, bar = float(d.max()), 4.0 * err32 * scale
    worst = int(d.flatten(1).max(dim=1).values.argmax())
    print(f"color_augment_ft {name}: max |kernel - fp64| = {err:.3e} (row {worst}: order {rows[2][worst].tolist()}, "
          f"sigma {float(rows[4][worst]):.3f}), float32 CPU evaluation {err32:.3e}, bar {bar:.3e}")
    assert err <= bar, (name, err, bar)


def test_color_augment_ft_every_halo_reflected():
    """S = 16, sigma = 2 on all 30 rows: every halo is 12 deep in a 16-pixel image, left and right, top and bottom"""
    x, factors, order, flags, _ = wc.ft_rows(16)
    rows = (x, factors, order, flags, torch.full((30,), 2.0))
    _hold("S=16 sigma=2", rows, *wc.ft_reference_and_bar(rows))


def test_color_augment_ft_matches_fp64_restatement_on_the_fixed_cases():
    """S = 32, B = 30: all 24 orders, a skip row, identity and extreme factors, sigma in {0, 0.001, 0.34, 1, 2}
    (no blur, the blur that changes nothing, tap radii 4, 6 and 12), the five fixed images"""
    rows, ref64, err32 = wc.ft_case(32)
    _hold("S=32", rows, ref64, err32)


def test_color_augment_ft_production_tiles():
    """S = 224, B = 4: the production tile grid (tile seams inside the image), sigma = (2, 1, 0.001, 0)"""
    rows = wc.ft_rows_224()
    _hold("S=224", rows, *wc.ft_reference_and_bar(rows))


def test_color_augment_ft_imagenet_constants():
    """the S = 32 rows normalised with the ImageNet constants: the bar of the [0, 1] case over the smallest std"""
    from ssl4gie_amd.ops import IMAGENET_MEAN, IMAGENET_STD
    rows, _, err32 = wc.ft_case(32)
    ref64 = wc.color_ft_ref(*rows, IMAGENET_MEAN, IMAGENET_STD, torch.float64)
    _hold("S=32 ImageNet mean / std", rows, ref64, err32, 1.0 / min(IMAGENET_STD), IMAGENET_MEAN, IMAGENET_STD)


def test_smallest_sigma_is_the_unblurred_result_bit_for_bit():
    """sigma = 0.001, the lower end of the reference's range: the centre weight is exactly 1 in fp32, the others 0"""
    from ssl4gie_amd import ops
    x, factors, order, flags, _ = wc.ft_rows(32)
    B = x.shape[0]
    tiny = _ft((x, factors, order, flags, torch.full((B,), 0.001)))
    none = _ft((x, factors, order, flags, torch.zeros(B)))
    assert torch.equal(tiny, none)
    # ... which is the existing stage's un-blurred result
    assert torch.equal(none, ops.color_augment(*(t.to(DEV) for t in (x, factors, order, flags, torch.zeros(B))), cc.ZERO3, cc.ONE3))


def _targets(S):
    """the three banks on the device, and each one's scaled float32 values on the CPU"""
    _, u8, u16, f32 = wc.warp_inputs(S)
    u16_dev = torch.from_numpy(u16.numpy().astype(np.uint16)).to(DEV)
    return (("uint8", u8.to(DEV), u8.to(torch.float32) / 255.0), ("uint16", u16_dev, u16.to(torch.float32) / 65535.0),
            ("float32", f32.to(DEV), f32))


@pytest.mark.parametrize("S", [16, 32, 224])
def test_paired_warp_matches_the_restatement_bit_for_bit(S):
    """the 21 fixed cases (identity, flips, right angles, scale 2 and 0.5, 12 draws from the segmentation ranges, a
    pure rotation), uint8, uint16 and float32 targets: not one differing pixel outside the tie mask"""
    from ssl4gie_amd import ops
    matrix, flip = wc.warp_cases(S)
    img = wc.warp_inputs(S)[0]
    B = img.shape[0]
    index = torch.randperm(B, generator=torch.Generator().manual_seed(S))             # the bank is read through the index
    for name, bank, scaled in _targets(S):
        out, tgt = ops.paired_warp(img.to(DEV), matrix.to(DEV), flip.to(DEV), FILL, bank, index.to(DEV), 0.5)
        assert out.dtype == tgt.dtype == torch.float32 and tuple(out.shape) == (B, 3, S, S) and tuple(tgt.shape) == (B, 1, S, S)
        ref, ref_tgt, tie = wc.warp_ref(img, scaled[index], matrix, flip, FILL, 0.5)
        share = tie.flatten(1).double().mean(dim=1)
        bad_img = (out.cpu().view(torch.int32) != ref.view(torch.int32)).any(dim=1) & ~tie
        bad_tgt = (tgt.cpu().view(torch.int32) != ref_tgt.view(torch.int32))[:, 0] & ~tie
        in_tie = int(((out.cpu() != ref).any(dim=1) & tie).sum())
        print(f"paired_warp S={S} {name}: {int(bad_img.sum())} image and {int(bad_tgt.sum())} target pixels differ outside "
              f"the tie mask, {in_tie} inside it; worst tie share {float(share.max()):.4f}")
        assert int(bad_img.sum()) == 0 and int(bad_tgt.sum()) == 0
        assert float(share.max()) <= wc.TIE_SHARE_MAX[S]
        # identity and flips: no tie, torch.flip exactly
        assert not bool(tie[:4].any())
        for b, dims in enumerate(((), (-1,), (-2,), (-2, -1))):
            assert torch.equal(out[b].cpu(), img[b].flip(dims) if dims else img[b])
            assert torch.equal(tgt[b, 0].cpu(), scaled[index[b]].flip(dims) if dims else scaled[index[b]])
    # int16 storage is read as uint16; no matrix is the identity, no flip is none; no target, no second output
    _, bank16, scaled16 = _targets(S)[1]
    out, tgt = ops.paired_warp(img.to(DEV), None, None, FILL, bank16.view(torch.int16), torch.arange(B, device=DEV))
    assert torch.equal(out.cpu(), img) and torch.equal(tgt[:, 0].cpu(), scaled16)
    alone = ops.paired_warp(img.to(DEV), matrix.to(DEV), flip.to(DEV), FILL)
    assert torch.is_tensor(alone) and torch.equal(alone, ops.paired_warp(img.to(DEV), matrix.to(DEV), flip.to(DEV), FILL, bank16,
                                                                         torch.arange(B, device=DEV))[0])


def test_warp_refusals_and_the_index_outside_the_bank():
    from ssl4gie_amd import _lib, ops
    S = 16
    matrix, flip = (t.to(DEV) for t in wc.warp_cases(S))
    img = wc.warp_inputs(S)[0].to(DEV)
    B = img.shape[0]
    _, bank, scaled = _targets(S)[0]
    # an index outside [0, n): that sample's target is all NaN (a bounds check, nothing is read), the rest is untouched
    index = torch.arange(B)
    index[3], index[9] = B, -1
    out, tgt = ops.paired_warp(img, matrix, flip, FILL, bank, index.to(DEV))
    good = ops.paired_warp(img, matrix, flip, FILL, bank, torch.arange(B, device=DEV))
    bad = torch.zeros(B, dtype=torch.bool)
    bad[[3, 9]] = True
    assert bool(torch.isnan(tgt[bad.to(DEV)]).all()) and torch.equal(tgt[~bad.to(DEV)], good[1][~bad.to(DEV)])
    assert torch.equal(out, good[0]) and bool(torch.isfinite(out).all())
    # the C entry point refuses an output that is, or overlaps, the input; the wrapper raises
    L = _lib.load()
    fill = (C.c_float * 3)(*FILL)
    buf = torch.zeros(2 * img.numel(), device=DEV)
    stream = torch.cuda.current_stream().cuda_stream
    for off in (0, 16, img.numel() - 4):
        assert L.ssl4gie_paired_warp(buf.data_ptr(), buf.data_ptr() + 4 * off, None, 0, 0, None, None, None, None, fill, 0.0,
                                     B, S, stream) == 1000
    assert not bool(buf.any())
    x, factors, order, flags, sigma = (t.to(DEV) for t in wc.ft_rows(S))
    with pytest.raises(ValueError, match="in place"):
        ops.color_augment_ft(x, factors, order, flags, sigma, out=x)
    with pytest.raises(ValueError, match="S >= 16"):
        ops.color_augment_ft(x[..., :12, :12].contiguous(), factors, order, flags, sigma)
    with pytest.raises(TypeError):
        ops.paired_warp(img, matrix, flip, FILL, bank.to(torch.int32), torch.arange(B, device=DEV))
    with pytest.raises(ValueError):
        ops.paired_warp(img, matrix, flip, FILL, bank)
    with pytest.raises(ValueError):
        ops.paired_warp(img, matrix[:, :5].contiguous(), flip, FILL)
    with pytest.raises(RuntimeError, match="contiguous"):
        ops.paired_warp(img, matrix, flip.repeat_interleave(2)[::2], FILL)
    out = torch.empty_like(x)
    assert ops.color_augment_ft(x, factors, order, flags, sigma, out=out) is out
    torch.cuda.synchronize()


def test_repeatable_and_independent_of_the_batch_position():
    """two launches give the same bits; a sample's result (its contrast mean included) does not depend on where in
    the batch it stands.  S = 96: two chunks per sample, six tiles."""
    from ssl4gie_amd import ops
    S = 96
    rows = list(wc.ft_rows(S, seed=5))
    rows[4] = rows[4].clone()
    rows[4][0] = rows[4][29] = 1.0
    for t in rows:
        t[29] = t[0]
    assert 1 in rows[2][0].tolist()
    a = _ft(rows)
    assert torch.equal(a, _ft(rows)) and torch.equal(a[0], a[29])
    perm = torch.arange(29, -1, -1)
    assert torch.equal(_ft(tuple(t[perm].contiguous() for t in rows)), a[perm])
    assert torch.equal(_ft(tuple(t[7:8].contiguous() for t in rows))[0], a[7])
    # the warp
    S = 32
    matrix, flip = wc.warp_cases(S)
    img = wc.warp_inputs(S)[0]
    B = img.shape[0]
    _, bank, _ = _targets(S)[1]
    index = torch.arange(B)
    run = lambda sel: ops.paired_warp(img[sel].to(DEV), matrix[sel].to(DEV), flip[sel].to(DEV), FILL, bank, index[sel].to(DEV))
    everything = torch.arange(B)
    a = run(everything)
    again = run(everything)
    assert torch.equal(a[0], again[0]) and torch.equal(a[1], again[1])
    perm = torch.arange(B - 1, -1, -1)
    p = run(perm)
    assert torch.equal(p[0], a[0][perm]) and torch.equal(p[1], a[1][perm])
    one = run(torch.tensor([11]))
    assert torch.equal(one[0][0], a[0][11]) and torch.equal(one[1][0], a[1][11])


def test_existing_color_augment_is_repeatable_bit_for_bit():
    """the MoCo colour stage shares its kernels' source with the finetune one: its S = 32 parity rows and an S = 224
    batch of the production case's kind, twice each, same bits (its parity tests hold its values)"""
    from ssl4gie_amd import ops
    rows32 = cc.parity_case(32)[0]
    x, factors, order, _, _ = wc.ft_rows_224()
    rows224 = (x, factors, order, torch.tensor([0, 2, 1, 2], dtype=torch.uint8), torch.tensor([2.0, 1.0, 0.34, 0.0]))
    for rows in (rows32, rows224):
        dev = tuple(t.to(DEV) for t in rows)
        a, b = ops.color_augment(*dev, cc.ZERO3, cc.ONE3), ops.color_augment(*dev, cc.ZERO3, cc.ONE3)
        assert torch.equal(a, b) and bool(torch.isfinite(a).all())


def test_unit_scale_view_sampling_is_normalize_u8_not_the_division():
    """what decides where FinetuneAugment takes its [0, 1] images from: view_sample_u8 with the whole image as its
    box, bilinear, mean 0, std 1, gives normalize_u8's bits — v times fp32 1 / 255 — and that is NOT v / 255 bit for
    bit (126 of the 256 levels differ), so the class uses normalize_u8 and says so"""
    from ssl4gie_amd import ops
    S = 32
    levels = torch.arange(256, dtype=torch.uint8).repeat(12)[: S * S * 3].view(1, S, S, 3).contiguous().to(DEV)
    box = torch.tensor([[0, 0, S, S]], dtype=torch.int32, device=DEV)
    view = ops.view_sample_u8(levels, torch.zeros(1, dtype=torch.int64, device=DEV), box, None, S, "bilinear", cc.ZERO3, cc.ONE3)
    norm = ops.normalize_u8(levels, cc.ZERO3, cc.ONE3)
    assert torch.equal(view, norm)
    # ToTensor's division, where the reference runs it: on the CPU (on the device torch itself divides a tensor by a
    # scalar as a multiplication by its reciprocal)
    division = levels.cpu().permute(0, 3, 1, 2).to(torch.float32) / 255.0
    assert not torch.equal(norm.cpu(), division) and float((norm.cpu() - division).abs().max()) < 2.0 ** -23


def _seeded(s):
    return torch.Generator(device=DEV).manual_seed(s)


def test_segmentation_recipe_through_the_device_loader():
    """FinetuneAugment.segmentation(32) over a 40-image bank with masks: (images, targets) per batch, the colour stage
    and the warp on the parameters the same seed draws; the image's fill region is exactly -1.0, the mask's exactly 0,
    and the two regions coincide pixel for pixel"""
    from ssl4gie_amd import ops
    from ssl4gie_amd.data import DeviceImageBank, DeviceLoader, FinetuneAugment
    device = torch.device(DEV)
    n, S, B = 40, 32, 8
    imgs = np.concatenate([cc.fixed_images_u8(S, seed=s)[:2] for s in range(n // 2)])
    rng = np.random.default_rng(3)
    masks = rng.integers(1, 256, size=(n, S, S), dtype=np.uint8)          # never 0: a 0 in the output is the fill
    bank = DeviceImageBank.from_uint8(imgs, device, targets=masks)
    loader = DeviceLoader(bank, B, sampler=torch.utils.data.SequentialSampler(bank),
                          transform=FinetuneAugment.segmentation(S, generator=_seeded(21)))
    assert len(loader) == 5
    twin = FinetuneAugment.segmentation(S, generator=_seeded(21))
    some_fill = 0
    for k, (images, targets) in enumerate(loader):
        assert tuple(images.shape) == (B, 3, S, S) and tuple(targets.shape) == (B, 1, S, S)
        assert images.dtype == targets.dtype == torch.float32 and images.device == targets.device == device
        assert bool(torch.isfinite(images).all()) and bool(torch.isfinite(targets).all())
        index = torch.arange(k * B, (k + 1) * B, device=device)
        factors, order, flags, sigma, flip, matrix = twin.draw(B, device)
        x = ops.normalize_u8(bank.images[index], cc.ZERO3, cc.ONE3)
        x = ops.color_augment_ft(x, factors, order, flags, sigma, twin.mean, twin.std)
        want = ops.paired_warp(x, matrix, flip, (-1.0, -1.0, -1.0), bank.targets, index, 0.0)
        assert torch.equal(images, want[0]) and torch.equal(targets, want[1])
        fill_img, fill_tgt = (images == -1.0).all(dim=1), targets[:, 0] == 0.0
        assert torch.equal(fill_img, fill_tgt)                            # the same map moved both
        # ... and it is the region the rule leaves outside, away from ties
        sx, sy = wc.source_coordinates(matrix.cpu(), S)
        outside = (torch.round(sx) < 0) | (torch.round(sx) > S - 1) | (torch.round(sy) < 0) | (torch.round(sy) > S - 1)
        tie = ((sx - torch.floor(sx) - 0.5).abs() <= wc.TIE_GUARD) | ((sy - torch.floor(sy) - 0.5).abs() <= wc.TIE_GUARD)
        assert not bool(((fill_img.cpu() != outside) & ~tie).any())
        assert bool((targets[:, 0][~fill_tgt] >= 1.0 / 255.0).all()) and float(targets.max()) <= 1.0
        some_fill += int(fill_img.sum())
    assert 0.05 < some_fill / (n * S * S) < 0.8


def test_depth_recipe_is_the_jitter_normalised_and_flipped():
    """FinetuneAugment.depth(32): no blur, no affine — the output is Normalize of the jittered image, flipped where the
    bits say so, and the target the bank's 16-bit row / 65535 through the same flips, bit for bit"""
    from ssl4gie_amd import ops
    from ssl4gie_amd.data import DeviceImageBank, FinetuneAugment
    device = torch.device(DEV)
    n, S = 12, 32
    imgs = np.concatenate([cc.fixed_images_u8(S, seed=s)[:3] for s in range(4)])
    depth = np.random.default_rng(4).integers(0, 65536, size=(n, S, S)).astype(np.uint16)
    bank = DeviceImageBank.from_uint8(imgs, device, targets=depth)
    B = 32
    index = (torch.arange(B, device=device) * 5) % n                        # every bank row, some of them thrice
    images, targets = FinetuneAugment.depth(S, generator=_seeded(8))(bank, index)
    factors, order, flags, sigma, flip, matrix = FinetuneAugment.depth(S, generator=_seeded(8)).draw(B, device)
    assert not bool(sigma.any()) and sorted(set(flip.tolist())) == [0, 1, 2, 3]
    x = ops.normalize_u8(bank.images[index], cc.ZERO3, cc.ONE3)
    jit = ops.color_augment(x, factors, order, flags, sigma)              # the existing stage: jitter + Normalize
    rows = torch.from_numpy(depth.astype(np.float32))[index.cpu()] / 65535.0
    for b, bits in enumerate(flip.tolist()):
        dims = [d for d, bit in ((-1, 1), (-2, 2)) if bits & bit]
        assert torch.equal(images[b], jit[b].flip(dims) if dims else jit[b])
        assert torch.equal(targets[b, 0].cpu(), rows[b].flip(dims) if dims else rows[b])
    # and the jitter is the restatement's, under the colour stage's bar
    cpu_rows = (x.cpu(), factors.cpu(), order.cpu(), flags.cpu(), sigma.cpu())
    ref64, err32 = wc.ft_reference_and_bar(cpu_rows, ops.IMAGENET_MEAN, ops.IMAGENET_STD)
    assert float((jit.cpu().double() - ref64).abs().max()) <= 4.0 * err32
    # classification: rotation alone, black fill in normalised space
    t = FinetuneAugment.classification(S, generator=_seeded(9))
    out = t(DeviceImageBank.from_uint8(imgs, device), index)
    assert torch.is_tensor(out) and tuple(out.shape) == (B, 3, S, S)
    corner = out[:, :, 0, 0].cpu()
    black = torch.tensor(t.fill, dtype=torch.float32)
    assert bool((corner == black).all(dim=1).any()) and abs(t.fill[0] + 0.485 / 0.229) < 1e-12
