"""CPU: pins tests/warp_checks.py — the restatement the GPU tests of ssl4gie_color_augment_ft and ssl4gie_paired_warp
trust — against torch's own ops (reflect pad + conv2d; torchvision's tensor path of TF.affine rebuilt from
grid_sample), its fixed cases against what they claim, and the rotation against PIL."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import colour_checks as cc
import warp_checks as wc


@pytest.mark.parametrize("S", [16, 32])
def test_blur25_is_reflect_pad_plus_depthwise_conv2d(S):
    """transforms.GaussianBlur((25, 25)) on its tensor path: the kernel on linspace(-12, 12, 25), pdf =
    exp(-0.5 (x / sigma)^2) normalised, its outer product, F.pad(mode="reflect") by 12, conv2d(groups=3)"""
    x = wc.warp_inputs(S)[3][:3].to(torch.float64)                     # [3, S, S] noise in [0, 1)
    for sigma in (0.001, 0.3, 1.0, 2.0):
        sigma32 = torch.tensor(sigma, dtype=torch.float32)
        t = torch.linspace(-12.0, 12.0, 25, dtype=torch.float64)
        pdf = torch.exp(-0.5 * (t / sigma32.to(torch.float64)).pow(2))
        k1 = pdf / pdf.sum()
        k2 = (k1[:, None] * k1[None, :]).expand(3, 1, 25, 25)
        ref = F.conv2d(F.pad(x[None], (12, 12, 12, 12), mode="reflect"), k2, groups=3)[0]
        got = wc.blur25(x, sigma32, torch.float64)
        assert got.dtype == torch.float64 and float((got - ref).abs().max()) <= 1e-12, sigma
    assert torch.equal(wc.blur25(x, torch.tensor(0.001), torch.float64), x)    # centre weight 1, the rest 0
    assert torch.equal(wc.blur25(x.float(), torch.tensor(0.001)), x.float())


def test_color_ft_ref_is_color_ref_with_the_other_blur():
    rows = wc.ft_rows(16)
    x, factors, order, flags, sigma = rows
    assert not bool(flags.any()) and sorted(set(sigma.tolist())) == sorted(np.float32(wc.FT_SIGMAS).tolist())
    ref = wc.color_ft_ref(*rows)
    plain, _ = cc.color_ref(x, factors, order, flags, torch.zeros_like(sigma))
    off = sigma <= 0.001                                                # no blur, or the one that changes nothing
    assert torch.equal(ref[off], plain[off]) and not torch.equal(ref[~off], plain[~off])
    b = int(torch.nonzero(sigma == 2.0)[0])
    assert torch.equal(ref[b], wc.blur25(plain[b], sigma[b]))
    m, s = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
    normed = wc.color_ft_ref(*rows, m, s)
    back = normed * torch.tensor(s, dtype=torch.float64).view(3, 1, 1) + torch.tensor(m, dtype=torch.float64).view(3, 1, 1)
    assert float((back - ref).abs().max()) < 1e-14


def _torchvision_tensor_affine(img, matrix32, flip, fill):
    """TF.hflip / TF.vflip where the bits say so, then TF.affine's tensor path: _gen_affine_grid (float32 base grid
    linspace(-S/2 + 0.5, S/2 - 0.5, S), bmm with theta^T / (0.5 S)) and _apply_grid_transform (grid_sample(nearest,
    zeros, align_corners=False) on the image and a ones mask, fill where the mask < 0.5)"""
    B, C, S, _ = img.shape
    x = img.clone()
    for b in range(B):
        if int(flip[b]) & 1:
            x[b] = x[b].flip(-1)
        if int(flip[b]) & 2:
            x[b] = x[b].flip(-2)
    theta = matrix32.view(B, 2, 3)
    lin = torch.linspace(-S * 0.5 + 0.5, S * 0.5 - 0.5, S, dtype=torch.float32)
    base = torch.empty(1, S, S, 3, dtype=torch.float32)
    base[..., 0] = lin.view(1, 1, S)
    base[..., 1] = lin.view(1, S, 1)
    base[..., 2] = 1.0
    rescaled = theta.transpose(1, 2) / torch.tensor([0.5 * S, 0.5 * S], dtype=torch.float32)
    grid = base.view(1, S * S, 3).expand(B, -1, -1).bmm(rescaled).view(B, S, S, 2)
    both = torch.cat([x, torch.ones(B, 1, S, S, dtype=x.dtype)], dim=1)
    out = F.grid_sample(both, grid, mode="nearest", padding_mode="zeros", align_corners=False)
    mask = out[:, -1:] < 0.5
    return torch.where(mask, torch.tensor(fill, dtype=x.dtype).view(1, C, 1, 1), out[:, :-1])


@pytest.mark.parametrize("S", [16, 32, 224])
def test_warp_ref_is_torchvisions_tensor_path_outside_the_tie_guard(S):
    """the fixed cases and 40 further draws from the segmentation ranges: not one differing pixel outside the tie
    mask, and the tie mask within its cap for every sample"""
    rng = np.random.default_rng(5)
    t = S / 8.0
    extra = [wc.inverse_affine(rng.uniform(-180, 180), rng.uniform(-t, t), rng.uniform(-t, t), rng.uniform(0.5, 1.5),
                               rng.uniform(-22.5, 22.5)) for _ in range(40)]
    matrix = torch.cat([wc.warp_cases(S)[0], torch.tensor(extra, dtype=torch.float64).to(torch.float32)])
    flip = torch.cat([wc.warp_cases(S)[1], torch.from_numpy(rng.integers(0, 4, 40).astype(np.uint8))])
    B = matrix.shape[0]
    g = torch.Generator().manual_seed(S)
    img = torch.randn(B, 3, S, S, generator=g)
    fill = (-1.0, -1.0, -1.0)
    ref, _, tie = wc.warp_ref(img, None, matrix, flip, fill)
    tv = _torchvision_tensor_affine(img, matrix, flip, fill)
    differ = (ref != tv).any(dim=1)
    share = tie.flatten(1).double().mean(dim=1)
    print(f"S={S}: {int(differ.sum())} differing pixels, {int((differ & ~tie).sum())} outside the guard; "
          f"worst tie share {float(share.max()):.4f}")
    assert int((differ & ~tie).sum()) == 0
    assert float(share.max()) <= wc.TIE_SHARE_MAX[S]


@pytest.mark.parametrize("S", [16, 32, 224])
def test_fixed_warp_cases_cover_what_they_claim(S):
    matrix, flip = wc.warp_cases(S)
    names = wc.CASE_NAMES
    assert matrix.dtype == torch.float32 and tuple(matrix.shape) == (len(names), 6) and len(names) == 21
    assert flip.dtype == torch.uint8 and flip[:4].tolist() == [0, 1, 2, 3]
    assert sorted(set(flip[8:20].tolist())) == [0, 1, 2, 3]
    img, u8, u16, f32 = wc.warp_inputs(S)
    out, tgt, tie = wc.warp_ref(img, u8, matrix, flip, (-1.0, -1.0, -1.0), 0)
    share = tie.flatten(1).double().mean(dim=1)
    assert float(share.max()) <= wc.TIE_SHARE_MAX[S], (names[int(share.argmax())], float(share.max()))
    assert not bool(tie[:6].any())                                     # identity, flips, 90 and 180 degrees: no tie
    # identity and flips are torch.flip, of the image and of the target alike
    for b, dims in enumerate(((), (-1,), (-2,), (-2, -1))):
        assert torch.equal(out[b], img[b].flip(dims) if dims else img[b])
        assert torch.equal(tgt[b, 0], u8[b].flip(dims) if dims else u8[b])
    # the right angles are rot90 / a point reflection: a permutation, nothing filled
    assert torch.equal(out[4], torch.rot90(img[4], 1, (-2, -1))) or torch.equal(out[4], torch.rot90(img[4], -1, (-2, -1)))
    assert torch.equal(out[5], img[5].flip((-2, -1)))
    # scale 2 shows the central half, every source pixel 2 x 2 times; scale 0.5 leaves a filled frame
    q = S // 4
    assert torch.equal(out[6], img[6][:, q:S - q, q:S - q].repeat_interleave(2, 1).repeat_interleave(2, 2))
    filled = (out[7] == -1.0).all(dim=0)
    assert 0.70 < float(filled.double().mean()) < 0.80 and not bool(filled[q + 1:S - q - 1, q + 1:S - q - 1].any())
    assert bool((tgt[7, 0][filled] == 0).all())
    # the generic rows: rotated, sheared, scaled (no row is a permutation of the axes) and partly filled
    for b in range(8, 21):
        assert float(matrix[b, 1].abs()) > 1e-3 and float(matrix[b, 3].abs()) > 1e-3, names[b]
    assert sum(bool((out[b] == -1.0).all(dim=0).any()) for b in range(8, 20)) >= 6
    assert float((matrix[20, [0, 1, 3, 4]].double().pow(2).sum() - 2.0).abs()) < 1e-6 and not bool(matrix[20, [2, 5]].any())


def test_rotation_against_pil_alarm():
    """ALARM, not parity: warp_ref with the matrix of TF.rotate(angle) = affine_matrices(-angle) against PIL's
    Image.rotate(angle) (nearest, black fill) — what Classification's RandomRotation runs — on an 8-bit noise image
    at S = 224.  PIL steps through the source in 16.16 fixed point, so it lands on the neighbouring pixel for source
    coordinates well beyond the 1e-3 tie guard.  Measured over the 64 angles below: worst per-image share of
    differing pixels 0.187 %, mean 0.103 %; outside the tie guard worst 0.042 %.  The gate is 2 x the worst measured
    share.  A wrong sign or a wrong centre in the matrix gives tens of per cent."""
    from PIL import Image
    from ssl4gie_amd.data import affine_matrices
    S = 224
    rng = np.random.default_rng(11)
    noise = rng.integers(1, 256, size=(S, S), dtype=np.uint8)          # no 0: black is the fill
    angles = rng.uniform(-180.0, 180.0, 64)
    matrix = affine_matrices(torch.from_numpy(-angles))
    img = torch.from_numpy(noise).view(1, 1, S, S).expand(64, 3, S, S)
    ref, _, tie = wc.warp_ref(img, None, matrix, None, (0, 0, 0))
    pil = torch.from_numpy(np.stack([np.asarray(Image.fromarray(noise).rotate(float(a))) for a in angles]))
    differ = ref[:, 0] != pil
    share = differ.flatten(1).double().mean(dim=1)
    outside = (differ & ~tie).flatten(1).double().mean(dim=1)
    print(f"rotation against PIL: worst share {float(share.max()):.5f}, mean {float(share.mean()):.5f}, outside the "
          f"tie guard worst {float(outside.max()):.5f}")
    assert float(share.max()) <= 2.0 * 0.00187
    assert float(share.max()) < 0.01
