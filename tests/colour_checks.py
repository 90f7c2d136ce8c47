"""Restatement, in torch ops, of the rule of ssl4gie_color_augment (include/ssl4gie_hip.h), and the fixed cases the
CPU and GPU tests share.  Not a test module: tests/test_colour_checks_cpu.py pins it against PIL, one op at a time;
tests/test_gpu_color_augment.py holds the kernel to its float64 evaluation, with a bar taken from its own float32
evaluation.

The rule, per sample b, on x = clamp(input, 0, 1), three channels per pixel:
  1. jitter: order[b] holds four op ids applied left to right; an id above 3 (255 by convention) is a skip, an id
     appears at most once.  blend(a, d, f) = clamp(f a + (1 - f) d, 0, 1); gray(x) = 0.299 r + 0.587 g + 0.114 b
     (PIL's "L" weights); f = factors[b][id]:
       0 brightness  blend(x, 0, f)
       1 contrast    blend(x, m, f), m = the mean of gray over the sample's whole current image (after the ops that
                     precede contrast in its order)
       2 saturation  blend(x, gray(x), f) per pixel
       3 hue         rgb -> hsv, h <- (h + f) mod 1, hsv -> rgb: the colorsys formulas in floating point as
                     torchvision's tensor path writes them, p, q, t clamped to [0, 1]; max == min keeps its value
  2. flags[b] & 1: all three channels <- gray(x)
  3. sigma[b] > 0: separable true Gaussian, R = min(ceil(3 sigma), 6), sigma being the float32 value it is stored as;
     weights exp(-k^2 / 2 sigma^2), k in [-R, R], over their sum; horizontal pass, then vertical; symmetric edges
     (index -1 - i reads i, S + i reads S - 1 - i)
  4. flags[b] & 2: x >= 128 / 255 -> 1 - x
  5. (x - mean[c]) / std[c]
No rounding to integer levels between the ops."""
import functools
import itertools
import math

import numpy as np
import torch

SKIP = 255
SOLARIZE_AT = 128.0 / 255.0
SOLARIZE_GUARD = 1e-5          # elements this close to the threshold (float64, pre-solarize) are not compared
SOLARIZE_EXCLUDED_MAX = 1e-3   # ... and may be at most this share of the solarized samples' elements
SIGMAS = (0.0, 0.1, 0.34, 1.0, 2.0)    # R = 0, 1, 2, 3, 6
ZERO3, ONE3 = (0.0, 0.0, 0.0), (1.0, 1.0, 1.0)


def gray(x):
    """[..., 3, H, W] -> [..., 1, H, W]"""
    return 0.299 * x[..., 0:1, :, :] + 0.587 * x[..., 1:2, :, :] + 0.114 * x[..., 2:3, :, :]


def blend(a, d, f):
    return (f * a + (1.0 - f) * d).clamp(0.0, 1.0)


def hue_shift(x, f):
    """[3, H, W]; torchvision's _rgb2hsv / _hsv2rgb, statement for statement"""
    r, g, b = x[0], x[1], x[2]
    maxc, minc = x.max(dim=0).values, x.min(dim=0).values
    eqc = maxc == minc
    cr = maxc - minc
    ones = torch.ones_like(maxc)
    s = cr / torch.where(eqc, ones, maxc)
    cr_divisor = torch.where(eqc, ones, cr)
    rc, gc, bc = (maxc - r) / cr_divisor, (maxc - g) / cr_divisor, (maxc - b) / cr_divisor
    hr = (maxc == r) * (bc - gc)
    hg = ((maxc == g) & (maxc != r)) * (2.0 + rc - bc)
    hb = ((maxc != g) & (maxc != r)) * (4.0 + gc - rc)
    h = torch.fmod((hr + hg + hb) / 6.0 + 1.0, 1.0)
    h = torch.remainder(h + f, 1.0)
    v = maxc
    i = torch.floor(h * 6.0)
    fr = h * 6.0 - i
    i = i.to(torch.int64) % 6
    p = (v * (1.0 - s)).clamp(0.0, 1.0)
    q = (v * (1.0 - fr * s)).clamp(0.0, 1.0)
    t = (v * (1.0 - (1.0 - fr) * s)).clamp(0.0, 1.0)
    table = torch.stack([torch.stack([v, q, p, p, t, v]), torch.stack([t, v, v, q, p, p]),
                         torch.stack([p, p, t, v, v, q])])            # [3, 6, H, W]
    out = table.gather(1, i.expand(3, 1, *i.shape)).squeeze(1)
    return torch.where(eqc, x, out)                                    # max == min keeps its value


def radius(sigma32):
    """R of a float32 sigma: ceil(3 sigma) on the exact value, at most 6"""
    return min(int(math.ceil(3.0 * float(sigma32))), 6)


def gaussian_weights(sigma, R, dtype):
    k = torch.arange(-R, R + 1, dtype=dtype)
    w = torch.exp(-(k * k) / (2.0 * sigma * sigma))
    return w / w.sum()


def symmetric_index(S, R):
    i = np.arange(-R, S + R)
    return torch.from_numpy(np.where(i < 0, -1 - i, np.where(i >= S, 2 * S - 1 - i, i)))


def blur(x, sigma, R):
    """[3, S, S], horizontal pass then vertical pass; sigma a 0-dim tensor of x's dtype"""
    S = x.shape[-1]
    w = gaussian_weights(sigma, R, x.dtype)
    idx = symmetric_index(S, R)
    xp = x[:, :, idx]
    x = sum(w[k] * xp[:, :, k:k + S] for k in range(2 * R + 1))
    xp = x[:, idx, :]
    return sum(w[k] * xp[:, k:k + S, :] for k in range(2 * R + 1))


def color_ref(x, factors, order, flags, sigma, mean=ZERO3, std=ONE3, dtype=torch.float64):
    """The rule, evaluated on the CPU in `dtype` (float64 or float32).  x [B, 3, S, S]; factors float32 [B, 4];
    order uint8 [B, 4]; flags uint8 [B]; sigma float32 [B].  Returns (out, pre): the result and the values just
    before the solarize step, both [B, 3, S, S] in `dtype`."""
    x = x.detach().cpu().to(dtype).clamp(0.0, 1.0)
    factors, sigma = factors.detach().cpu().to(torch.float32), sigma.detach().cpu().to(torch.float32)
    order, flags = order.detach().cpu().tolist(), flags.detach().cpu().tolist()
    m_ = torch.tensor(mean, dtype=dtype).view(3, 1, 1)
    s_ = torch.tensor(std, dtype=dtype).view(3, 1, 1)
    outs, pres = [], []
    for b in range(x.shape[0]):
        v = x[b]
        for op in order[b]:
            if op > 3:
                continue
            f = factors[b, op].to(dtype)
            if op == 0:
                v = blend(v, 0.0, f)
            elif op == 1:
                v = blend(v, gray(v).mean(), f)
            elif op == 2:
                v = blend(v, gray(v), f)
            else:
                v = hue_shift(v, f)
        if flags[b] & 1:
            v = gray(v).expand(3, -1, -1)
        if float(sigma[b]) > 0.0:
            v = blur(v, sigma[b].to(dtype), radius(sigma[b]))
        pres.append(v)
        if flags[b] & 2:
            v = torch.where(v >= SOLARIZE_AT, 1.0 - v, v)
        outs.append((v - m_) / s_)
    return torch.stack(outs), torch.stack(pres)


# ---- fixed inputs -------------------------------------------------------------------------------------------------
IMAGE_NAMES = ("noise", "smooth", "gray", "black", "white")


def fixed_images_u8(S, seed=0):
    """uint8 [5, S, S, 3]: 8-bit noise, a smooth image, a gray image (max == min: the hue branch), black, white"""
    rng = np.random.default_rng(seed)
    y, x = np.meshgrid(np.arange(S) / (S - 1), np.arange(S) / (S - 1), indexing="ij")
    smooth = np.stack([0.5 + 0.5 * np.sin(2.1 * x + 0.3) * np.cos(1.3 * y), 0.2 + 0.7 * x * y, 0.9 - 0.8 * (x - y) ** 2], axis=2)
    g = rng.integers(0, 256, size=(S, S, 1), dtype=np.uint8).repeat(3, axis=2)
    return np.stack([rng.integers(0, 256, size=(S, S, 3), dtype=np.uint8),
                     np.clip(np.rint(smooth * 255.0), 0, 255).astype(np.uint8), g,
                     np.zeros((S, S, 3), np.uint8), np.full((S, S, 3), 255, np.uint8)])


def fixed_images(S, seed=0):
    """float32 [5, 3, S, S] in [0, 1]"""
    return (torch.from_numpy(fixed_images_u8(S, seed)).permute(0, 3, 1, 2).to(torch.float32) / 255.0).contiguous()


PERMS = tuple(itertools.permutations(range(4)))     # all 24 orders


def parity_rows(S, seed=0):
    """The B = 30 rows of the parity tests: x float32 [30, 3, S, S], factors, order, flags, sigma.
    Rows 0..23 carry the 24 orders, row 24 is a skip row, row 25 identity factors with a real order, rows 26..29
    mid-range factors; the extreme factors (0.6 / 1.4, 0.6 / 1.4, 0.8 / 1.2, -0.1 / 0.1) alternate over rows
    0..23, the flags cycle through 0..3, sigma through SIGMAS (shifted every five rows, so that every sigma meets
    every image), the image through the five fixed ones."""
    imgs = fixed_images(S, seed)
    rng = np.random.default_rng(seed + 1)
    B = 30
    factors = np.zeros((B, 4), np.float32)
    order = np.zeros((B, 4), np.uint8)
    for i in range(B):
        factors[i] = (0.6 if i & 1 else 1.4, 1.4 if i & 2 else 0.6, 0.8 if i & 4 else 1.2, 0.1 if i & 8 else -0.1)
        order[i] = PERMS[(7 * i) % 24]
    for i in range(24):
        order[i] = PERMS[i]
    order[24], factors[24] = SKIP, (1.0, 1.0, 1.0, 0.0)
    order[25], factors[25] = (0, 1, 2, 3), (1.0, 1.0, 1.0, 0.0)
    for i in range(26, B):
        factors[i] = (rng.uniform(0.6, 1.4), rng.uniform(0.6, 1.4), rng.uniform(0.8, 1.2), rng.uniform(-0.1, 0.1))
    flags = np.array([i % 4 for i in range(B)], np.uint8)
    sigma = np.array([SIGMAS[(i + i // 5) % 5] for i in range(B)], np.float32)
    x = imgs[[i % 5 for i in range(B)]].contiguous()
    return x, torch.from_numpy(factors), torch.from_numpy(order), torch.from_numpy(flags), torch.from_numpy(sigma)


def compare_mask(pre64, flags):
    """bool [B, 3, S, S]: the elements to compare — all but those of solarized samples whose float64 pre-solarize
    value lies within SOLARIZE_GUARD of the threshold; and the excluded share of the solarized samples' elements"""
    sol = (torch.as_tensor(flags).view(-1, 1, 1, 1) & 2) != 0
    near = sol & ((pre64 - SOLARIZE_AT).abs() <= SOLARIZE_GUARD)
    n_sol = int(sol.sum()) * pre64[0].numel()
    return ~near, (float(near.sum()) / n_sol if n_sol else 0.0)


@functools.lru_cache(maxsize=None)
def parity_case(S, mean=ZERO3, std=ONE3, seed=0):
    """(inputs, float64 result, mask of compared elements, excluded share, float32-evaluation error): computed
    once per (S, mean, std), shared by the tests, never modified"""
    rows = parity_rows(S, seed)
    return (rows,) + reference_and_bar(rows, mean, std)


def reference_and_bar(rows, mean=ZERO3, std=ONE3):
    """float64 result, compare mask, excluded share, and max |float32 evaluation - float64 evaluation| over the
    compared elements"""
    ref64, pre64 = color_ref(*rows, mean, std, torch.float64)
    ref32, _ = color_ref(*rows, mean, std, torch.float32)
    mask, share = compare_mask(pre64, rows[3])
    err32 = float(((ref32.to(torch.float64) - ref64).abs() * mask).max())
    return ref64, mask, share, err32
