"""Restatement, in torch ops, of the rules of ssl4gie_color_augment_ft and ssl4gie_paired_warp (include/ssl4gie_hip.h),
and the fixed cases the CPU and GPU tests share.  Not a test module: tests/test_warp_checks_cpu.py pins it against
torch's own reflect pad + conv2d, against torchvision's tensor path rebuilt from grid_sample, and against PIL;
tests/test_gpu_finetune_augment.py holds the kernels to it.

Colour stage: colour_checks' rule with step 3 replaced by the 25-tap blur of transforms.GaussianBlur((25, 25)):
k in [-12, 12], weights exp(-k^2 / 2 sigma^2) over their sum, horizontal pass then vertical, reflect edges (index -i
reads i, S - 1 + i reads S - 1 - i).

Warp: sample b, output pixel (i, j), c = (S - 1) / 2, xo = j - c, yo = i - c, m = matrix[b]:
  sx = m0 xo + m1 yo + m2 + c, sy = m3 xo + m4 yo + m5 + c, ix = rint(sx), iy = rint(sy) (half to even);
  outside [0, S)^2: the fill; otherwise ix <- S - 1 - ix where flip & 1, iy <- S - 1 - iy where flip & 2 (the flips
  happen BEFORE the affine, so they mirror the source), and the pixel is the source pixel.
Evaluated in float64 on the float32 matrix values as they are.  A pixel whose sx or sy lies within TIE_GUARD of a
half-integer may legitimately land on either neighbour in an fp32 evaluation (the kernel's, torchvision's): such
pixels are reported in a mask and not compared."""
import functools
import math

import numpy as np
import torch

import colour_checks as cc

FT_R = 12
TIE_GUARD = 1e-3
TIE_SHARE_MAX = {16: 0.04, 32: 0.04, 224: 0.02}     # of one sample's pixels
FT_SIGMAS = (0.0, 0.001, 0.34, 1.0, 2.0)
SEG_RANGES = dict(angle=180.0, translate=1.0 / 8.0, scale=(0.5, 1.5), shear=22.5)


# ---- colour stage -------------------------------------------------------------------------------------------------
def gaussian25(sigma, dtype):
    k = torch.arange(-FT_R, FT_R + 1, dtype=dtype)
    w = torch.exp(-(k * k) / (2.0 * sigma * sigma))
    return w / w.sum()


def reflect_index(S, R=FT_R):
    i = np.arange(-R, S + R)
    return torch.from_numpy(np.where(i < 0, -i, np.where(i >= S, 2 * S - 2 - i, i)))


def blur25(x, sigma, dtype=None):
    """[3, S, S] -> [3, S, S]: horizontal pass, then vertical; sigma a number or 0-dim tensor, taken to `dtype`
    (default: x's)"""
    dtype = x.dtype if dtype is None else dtype
    x = x.to(dtype)
    S = x.shape[-1]
    w = gaussian25(torch.as_tensor(sigma).to(dtype), dtype)
    idx = reflect_index(S)
    xp = x[:, :, idx]
    x = sum(w[k] * xp[:, :, k:k + S] for k in range(2 * FT_R + 1))
    xp = x[:, idx, :]
    return sum(w[k] * xp[:, k:k + S, :] for k in range(2 * FT_R + 1))


def color_ft_ref(x, factors, order, flags, sigma, mean=cc.ZERO3, std=cc.ONE3, dtype=torch.float64):
    """colour_checks.color_ref with blur25 as step 3: its steps 1 and 2 are taken from color_ref itself (its `pre`
    output with the blur switched off), steps 3', 4 and 5 follow here.  Returns [B, 3, S, S] in `dtype`."""
    sigma = sigma.detach().cpu().to(torch.float32)
    flags_l = flags.detach().cpu().tolist()
    _, pre = cc.color_ref(x, factors, order, flags, torch.zeros_like(sigma), cc.ZERO3, cc.ONE3, dtype)
    m_ = torch.tensor(mean, dtype=dtype).view(3, 1, 1)
    s_ = torch.tensor(std, dtype=dtype).view(3, 1, 1)
    outs = []
    for b in range(pre.shape[0]):
        v = pre[b]
        if float(sigma[b]) > 0.0:
            v = blur25(v, sigma[b])
        if flags_l[b] & 2:
            v = torch.where(v >= cc.SOLARIZE_AT, 1.0 - v, v)
        outs.append((v - m_) / s_)
    return torch.stack(outs)


def ft_reference_and_bar(rows, mean=cc.ZERO3, std=cc.ONE3):
    """float64 result and max |float32 evaluation - float64 evaluation| of the restatement on the same rows"""
    ref64 = color_ft_ref(*rows, mean, std, torch.float64)
    ref32 = color_ft_ref(*rows, mean, std, torch.float32)
    return ref64, float((ref32.to(torch.float64) - ref64).abs().max())


def ft_rows(S, sigmas=FT_SIGMAS, seed=0):
    """colour_checks.parity_rows' images, orders and factors, no grayscale or solarize bits (the finetune loaders
    have neither), sigma cycling through `sigmas` (shifted every five rows, so that every sigma meets every image)"""
    x, factors, order, _, _ = cc.parity_rows(S, seed)
    B = x.shape[0]
    sigma = torch.tensor([sigmas[(i + i // 5) % len(sigmas)] for i in range(B)], dtype=torch.float32)
    return x, factors, order, torch.zeros(B, dtype=torch.uint8), sigma


@functools.lru_cache(maxsize=None)
def ft_case(S, sigmas=FT_SIGMAS, mean=cc.ZERO3, std=cc.ONE3):
    """(rows, float64 result, float32-evaluation error): computed once, shared by the tests, never modified"""
    rows = ft_rows(S, sigmas)
    return (rows,) + ft_reference_and_bar(rows, mean, std)


def ft_rows_224():
    """S = 224, B = 4: the production tile grid, sigma = (2, 1, 0.001, 0); the images and jitter of
    test_gpu_color_augment's production case, without its flags"""
    S = 224
    g = torch.Generator().manual_seed(3)
    noise = torch.randint(0, 256, (2, 3, S, S), generator=g).to(torch.float32) / 255.0
    yy, xx = torch.meshgrid(torch.linspace(0, 1, S), torch.linspace(0, 1, S), indexing="ij")
    smooth = torch.stack([0.5 + 0.5 * torch.sin(7.0 * xx) * torch.cos(5.0 * yy), 0.1 + 0.8 * xx * yy, 0.9 - 0.8 * (xx - yy) ** 2])
    x = torch.stack([noise[0], smooth, noise[1], smooth]).contiguous()
    factors = torch.tensor([[1.4, 0.6, 1.2, 0.1], [0.6, 1.4, 0.8, -0.1], [1.2, 1.3, 0.9, 0.05], [0.8, 1.4, 1.1, -0.07]],
                           dtype=torch.float32)
    order = torch.tensor([[0, 2, 3, 1], [3, 1, 2, 0], [2, 0, 1, 3], [1, 0, 3, 2]], dtype=torch.uint8)
    return x, factors, order, torch.zeros(4, dtype=torch.uint8), torch.tensor([2.0, 1.0, 0.001, 0.0])


# ---- warp ---------------------------------------------------------------------------------------------------------
def inverse_affine(angle, tx, ty, scale, shear):
    """torchvision's _get_inverse_affine_matrix(center=(0, 0), angle, (tx, ty), scale, (shear, 0)) in Python floats"""
    rot, sx, sy = math.radians(angle), math.radians(shear), 0.0
    a = math.cos(rot - sy) / math.cos(sy)
    b = -math.cos(rot - sy) * math.tan(sx) / math.cos(sy) - math.sin(rot)
    c = math.sin(rot - sy) / math.cos(sy)
    d = -math.sin(rot - sy) * math.tan(sx) / math.cos(sy) + math.cos(rot)
    m = [d / scale, -b / scale, 0.0, -c / scale, a / scale, 0.0]
    m[2] += m[0] * -tx + m[1] * -ty
    m[5] += m[3] * -tx + m[4] * -ty
    return m


def source_coordinates(matrix32, S):
    """float64 (sx, sy), each [B, S, S], of the float32 matrix values as they are"""
    m = matrix32.detach().cpu().to(torch.float64)
    c = (S - 1) / 2.0
    o = torch.arange(S, dtype=torch.float64) - c
    xo, yo = o.view(1, 1, S), o.view(1, S, 1)
    e = lambda k: m[:, k].view(-1, 1, 1)
    return e(0) * xo + e(1) * yo + e(2) + c, e(3) * xo + e(4) * yo + e(5) + c


def warp_ref(img, tgt, matrix32, flip, fill_img, fill_tgt=0.0):
    """img [B, 3, S, S], tgt [B, S, S] (already scaled) or None, matrix32 float32 [B, 6] or None, flip uint8 [B] or
    None.  Returns (img_out, tgt_out [B, 1, S, S] or None, tie bool [B, S, S]); values are moved, never computed
    with, so the outputs keep the inputs' dtypes and bits."""
    img = img.detach().cpu()
    B, _, S, _ = img.shape
    if matrix32 is None:
        matrix32 = torch.tensor([[1.0, 0.0, 0.0, 0.0, 1.0, 0.0]], dtype=torch.float32).repeat(B, 1)
    bits = torch.zeros(B, dtype=torch.int64) if flip is None else flip.detach().cpu().to(torch.int64)
    sx, sy = source_coordinates(matrix32, S)
    tie = ((sx - torch.floor(sx) - 0.5).abs() <= TIE_GUARD) | ((sy - torch.floor(sy) - 0.5).abs() <= TIE_GUARD)
    ix, iy = torch.round(sx), torch.round(sy)              # half to even
    inside = (ix >= 0) & (ix <= S - 1) & (iy >= 0) & (iy <= S - 1)
    ix = torch.where(inside, ix, torch.zeros_like(ix)).to(torch.int64)
    iy = torch.where(inside, iy, torch.zeros_like(iy)).to(torch.int64)
    ix = torch.where((bits & 1).view(-1, 1, 1) != 0, S - 1 - ix, ix)
    iy = torch.where((bits & 2).view(-1, 1, 1) != 0, S - 1 - iy, iy)
    flat = (iy * S + ix).view(B, 1, S * S)
    fill = torch.tensor(fill_img, dtype=img.dtype).view(1, 3, 1, 1)
    out = torch.where(inside.unsqueeze(1), img.reshape(B, 3, S * S).gather(2, flat.expand(B, 3, S * S)).view(B, 3, S, S), fill)
    tgt_out = None
    if tgt is not None:
        tgt = tgt.detach().cpu()
        moved = tgt.reshape(B, 1, S * S).gather(2, flat).view(B, 1, S, S)
        tgt_out = torch.where(inside.unsqueeze(1), moved, torch.tensor(fill_tgt, dtype=tgt.dtype))
    return out, tgt_out, tie


CASE_NAMES = ("identity", "hflip", "vflip", "hflip + vflip", "rotate 90", "rotate 180", "scale 2",
              "scale 0.5 + 1/8 px") + tuple(f"segmentation draw {i}" for i in range(12)) + ("rotation only",)


@functools.lru_cache(maxsize=None)
def warp_cases(S, seed=0):
    """(matrix float32 [21, 6], flip uint8 [21]) of CASE_NAMES.  The identity, flip and rotate rows have no tie: their
    source coordinates are integers.  A pure scale of 0.5 (inverse matrix 2 I) would put EVERY source coordinate on
    a half-integer (2 j - c), so that row carries a translation of an eighth of a pixel.  The segmentation draws
    come from SEG_RANGES at a fixed seed, their flip bits cycle through 0..3."""
    rng = np.random.default_rng(1000 + seed)
    rows = [([1.0, 0.0, 0.0, 0.0, 1.0, 0.0], f) for f in range(4)]
    rows += [([0.0, 1.0, 0.0, -1.0, 0.0, 0.0], 0), ([-1.0, 0.0, 0.0, 0.0, -1.0, 0.0], 0)]
    rows += [(inverse_affine(0.0, 0.0, 0.0, 2.0, 0.0), 0), (inverse_affine(0.0, 0.125, 0.125, 0.5, 0.0), 0)]
    t = SEG_RANGES["translate"] * S
    for i in range(12):
        rows.append((inverse_affine(rng.uniform(-180.0, 180.0), rng.uniform(-t, t), rng.uniform(-t, t),
                                    rng.uniform(*SEG_RANGES["scale"]), rng.uniform(-22.5, 22.5)), i % 4))
    rows.append((inverse_affine(-33.0, 0.0, 0.0, 1.0, 0.0), 1))
    assert len(rows) == len(CASE_NAMES)
    return (torch.tensor([r[0] for r in rows], dtype=torch.float64).to(torch.float32),
            torch.tensor([r[1] for r in rows], dtype=torch.uint8))


@functools.lru_cache(maxsize=None)
def warp_inputs(S, seed=0):
    """(img float32 [21, 3, S, S] in normalised space, u8 [21, S, S], u16 [21, S, S] as int32, f32 [21, S, S]): noise,
    so that a pixel taken from the wrong place shows"""
    B = len(CASE_NAMES)
    g = torch.Generator().manual_seed(77 + seed)
    img = torch.randn(B, 3, S, S, generator=g)
    u8 = torch.randint(0, 256, (B, S, S), generator=g, dtype=torch.int32).to(torch.uint8)
    u16 = torch.randint(0, 65536, (B, S, S), generator=g, dtype=torch.int32)
    f32 = torch.rand(B, S, S, generator=g)
    return img, u8, u16, f32
