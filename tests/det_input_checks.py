"""Restatement, in torch ops, of the rule of ssl4gie_det_color / ssl4gie_det_geometry / ssl4gie_det_boxes
(include/ssl4gie_hip.h), and the fixed cases the CPU and GPU tests share.  Not a test module:
tests/test_det_input_checks_cpu.py pins it against the reference's own dataset class (tests/golden/g21_det_loader.npz),
against F.interpolate and against warp_checks; tests/test_gpu_det_loader.py holds the kernels to it.

The rule, per sample, stored image S [H0][W0] uint8 HWC, decisions (r, h, v):
  1. colour (training only): colour_checks' jitter (rule step 1) and warp_checks' 25-tap reflect blur on the H0 x W0
     rectangle of x = float(v) / 255; no rounding to 8-bit levels, no normalisation;
  2. ToTensor: float(v) / 255, correctly rounded;
  3. r: T1[i][j] = S[j][W0 - 1 - i]; boxes (ymin, W0 - xmax, ymax, W0 - xmin);
  4. h: T2[i][j] = T1[i][W1 - 1 - j]; boxes' x (W1 - xmax, W1 - xmin);
  5. v: T3[i][j] = T2[H1 - 1 - i][j]; boxes' y (H1 - ymax, H1 - ymin);
  6. only when H1 > F or W1 > F: a zero row / column appended to an odd side, then the antialiased bicubic halving:
     output i reads inputs max(0, 2 i - 3) .. min(L, 2 i + 5) - 1 with Keys' a = -0.5 weights w((j - 2 i - 0.5) / 2)
     over their sum; boxes / 2;
  7. p1 = floor((F - W2) / 2), p2 = floor((F - H2) / 2): centre pad with black, (x - mean) / std; boxes += (p1, p2, p1, p2).
Box arithmetic is fp32, one operation per statement, in this order."""
import functools

import numpy as np
import torch

import colour_checks as cc
import warp_checks as wc

DYADIC = (-3.0, -9.0, 29.0, 111.0, 111.0, 29.0, -9.0, -3.0)     # / 256: the interior weights of step 6
COLOR_SHAPES = ((13, 13), (16, 40), (71, 93))


# ---- steps 2 - 7 ---------------------------------------------------------------------------------------------------
def to_tensor(img_u8, dtype=torch.float32):
    """uint8 [H, W, 3] (array or tensor) -> [3, H, W]: float32(v) / 255 as ToTensor computes it, then taken to `dtype`"""
    t = torch.as_tensor(np.asarray(img_u8)).permute(2, 0, 1).contiguous()
    return t.to(torch.float32).div(255).to(dtype)


def keys(x):
    """Keys' cubic convolution kernel with a = -0.5"""
    x = x.abs()
    return torch.where(x < 1.0, (1.5 * x - 2.5) * x * x + 1.0,
                       torch.where(x < 2.0, ((-0.5 * x + 2.5) * x - 4.0) * x + 2.0, torch.zeros_like(x)))


def halve_matrix(L, dtype):
    """[L / 2, L] (L even): row i holds the normalised weights of output i"""
    assert L % 2 == 0
    M = torch.zeros(L // 2, L, dtype=dtype)
    for i in range(L // 2):
        lo, hi = max(0, 2 * i - 3), min(L, 2 * i + 5)
        j = torch.arange(lo, hi, dtype=dtype)
        w = keys((j - 2 * i - 0.5) / 2.0)
        M[i, lo:hi] = w / w.sum()
    return M


def halve(x, dtype=None):
    """[3, H, W] -> [3, ceil(H / 2), ceil(W / 2)]: zero row / column onto an odd side, horizontal pass, then vertical"""
    dtype = x.dtype if dtype is None else dtype
    x = x.to(dtype)
    _, H, W = x.shape
    x = torch.nn.functional.pad(x, (0, W % 2, 0, H % 2))
    x = x @ halve_matrix(x.shape[2], dtype).T
    return (halve_matrix(x.shape[1], dtype) @ x)


def out_geometry(H0, W0, r, F):
    """(H1, W1, halve?, H2, W2, p1, p2)"""
    H1, W1 = (W0, H0) if r else (H0, W0)
    hv = H1 > F or W1 > F
    H2, W2 = ((H1 + 1) // 2, (W1 + 1) // 2) if hv else (H1, W1)
    return H1, W1, hv, H2, W2, (F - W2) // 2, (F - H2) // 2


def geometry_ref(x, dec, F, dtype=None, mean=cc.ZERO3, std=cc.ONE3):
    """steps 3 - 7 on x [3, H0, W0] -> [3, F, F] in `dtype` (default x's).  Without a halving and with the default
    mean / std values are only moved."""
    dtype = x.dtype if dtype is None else dtype
    r, h, v = (bool(d) for d in dec)
    x = x.to(dtype)
    _, H0, W0 = x.shape
    if r:
        x = x.transpose(1, 2).flip(1)          # T1[i][j] = S[j][W0 - 1 - i]
    if h:
        x = x.flip(2)
    if v:
        x = x.flip(1)
    _, _, hv, H2, W2, p1, p2 = out_geometry(H0, W0, r, F)
    if hv:
        x = halve(x)
    assert tuple(x.shape[1:]) == (H2, W2) and H2 <= F and W2 <= F
    out = torch.zeros(3, F, F, dtype=dtype)
    out[:, p2:p2 + H2, p1:p1 + W2] = x
    if tuple(mean) == cc.ZERO3 and tuple(std) == cc.ONE3:
        return out
    return (out - torch.tensor(mean, dtype=dtype).view(3, 1, 1)) / torch.tensor(std, dtype=dtype).view(3, 1, 1)


def boxes_ref(boxes, H0, W0, dec, F):
    """float32 [k, 4] -> float32 [k, 4]; every statement one float32 operation, in the rule's order"""
    b = torch.as_tensor(np.asarray(boxes), dtype=torch.float32).reshape(-1, 4).clone()
    r, h, v = (bool(d) for d in dec)
    H1, W1, hv, _, _, p1, p2 = out_geometry(H0, W0, r, F)
    if r:
        b = torch.stack([b[:, 1], W0 - b[:, 2], b[:, 3], W0 - b[:, 0]], dim=1)
    if h:
        b = torch.stack([W1 - b[:, 2], b[:, 1], W1 - b[:, 0], b[:, 3]], dim=1)
    if v:
        b = torch.stack([b[:, 0], H1 - b[:, 3], b[:, 2], H1 - b[:, 1]], dim=1)
    if hv:
        b = b / 2
    return b + torch.tensor([p1, p2, p1, p2], dtype=torch.float32)


def geom_bits(dec):
    """the kernels' geom byte: bit 0 hflip, bit 1 vflip, bit 2 rot90"""
    r, h, v = (int(bool(d)) for d in dec)
    return h + 2 * v + 4 * r


def bits_dec(bits):
    return (bits >> 2) & 1, bits & 1, (bits >> 1) & 1


# ---- step 1 on a rectangle -------------------------------------------------------------------------------------------
def blur25_rect(x, sigma, dtype=None):
    """warp_checks.blur25 with H and W in S's place on the two axes: [3, H, W] -> [3, H, W]"""
    dtype = x.dtype if dtype is None else dtype
    x = x.to(dtype)
    _, H, W = x.shape
    w = wc.gaussian25(torch.as_tensor(sigma).to(dtype), dtype)
    xp = x[:, :, wc.reflect_index(W)]
    x = sum(w[k] * xp[:, :, k:k + W] for k in range(2 * wc.FT_R + 1))
    xp = x[:, wc.reflect_index(H), :]
    return sum(w[k] * xp[:, k:k + H, :] for k in range(2 * wc.FT_R + 1))


def color_rect_ref(x, factors, order, sigma, dtype=torch.float64):
    """x [B, 3, H, W] in [0, 1] -> [B, 3, H, W] in `dtype`: colour_checks.color_ref's jitter (its steps 1 with the
    blur switched off; it is written for any H x W), then blur25_rect where sigma > 0.  No normalisation."""
    sigma = sigma.detach().cpu().to(torch.float32)
    zeros = torch.zeros(x.shape[0], dtype=torch.uint8)
    _, pre = cc.color_ref(x, factors, order, zeros, torch.zeros_like(sigma), cc.ZERO3, cc.ONE3, dtype)
    return torch.stack([blur25_rect(pre[b], sigma[b]) if float(sigma[b]) > 0.0 else pre[b] for b in range(pre.shape[0])])


def rect_images_u8(H, W, seed=0):
    """uint8 [5, H, W, 3]: colour_checks' five fixed images of size max(H, W), cut to H x W"""
    return np.ascontiguousarray(cc.fixed_images_u8(max(H, W), seed)[:, :H, :W])


@functools.lru_cache(maxsize=None)
def color_case(H, W):
    """(images uint8 [30, H, W, 3], factors, order, sigma, float64 result, float32-evaluation error) of the 30 parity
    rows of colour_checks (all 24 orders, a skip row) with warp_checks' sigmas; computed once, never modified"""
    _, factors, order, _, _ = cc.parity_rows(16)
    imgs = rect_images_u8(H, W)
    B = factors.shape[0]
    u8 = np.ascontiguousarray(imgs[[i % 5 for i in range(B)]])
    sigma = torch.tensor([wc.FT_SIGMAS[(i + i // 5) % len(wc.FT_SIGMAS)] for i in range(B)], dtype=torch.float32)
    x = torch.stack([to_tensor(u) for u in u8])
    ref64 = color_rect_ref(x, factors, order, sigma, torch.float64)
    ref32 = color_rect_ref(x, factors, order, sigma, torch.float32)
    return u8, factors, order, sigma, ref64, float((ref32.to(torch.float64) - ref64).abs().max())


# ---- the fixture -----------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def g21(path):
    """[(img uint8 [H, W, 3], boxes, dec (r, h, v), out_img [3, F, F], out_boxes)], F"""
    z = np.load(path)
    n = sum(1 for k in z.files if k.startswith("img/"))
    return [(z[f"img/{k}"], z[f"boxes/{k}"], tuple(int(d) for d in z[f"dec/{k}"]), z[f"out_img/{k}"], z[f"out_boxes/{k}"])
            for k in range(n)], int(z["fixed_size"])


def is_halved(img, dec, F):
    return out_geometry(img.shape[0], img.shape[1], dec[0], F)[2]


def halved_ref_and_err32(img_u8, dec, F):
    """for a case that IS halved: (float64 restatement [3, F, F] with mean 0 / std 1, max |torch's own float32 CPU
    F.interpolate - the float64 restatement| on the same turned image); the float64 halving is computed once"""
    t64 = turned(to_tensor(img_u8, torch.float64), dec)
    h64 = halve(t64)
    p = torch.nn.functional.pad(t64.to(torch.float32), (0, t64.shape[2] % 2, 0, t64.shape[1] % 2))
    got = torch.nn.functional.interpolate(p.unsqueeze(0), size=tuple(h64.shape[1:]), mode="bicubic", antialias=True,
                                          align_corners=False)[0]
    _, _, hv, H2, W2, p1, p2 = out_geometry(img_u8.shape[0], img_u8.shape[1], dec[0], F)
    assert hv and tuple(h64.shape[1:]) == (H2, W2)
    ref = torch.zeros(3, F, F, dtype=torch.float64)
    ref[:, p2:p2 + H2, p1:p1 + W2] = h64
    return ref, float((got.to(torch.float64) - h64).abs().max())


def interp_error32(x64_turned):
    """max |torch's own float32 CPU F.interpolate - the float64 restatement| on a turned, padded-to-even image"""
    x = x64_turned
    x = torch.nn.functional.pad(x, (0, x.shape[2] % 2, 0, x.shape[1] % 2))
    size = (x.shape[1] // 2, x.shape[2] // 2)
    got = torch.nn.functional.interpolate(x.to(torch.float32).unsqueeze(0), size=size, mode="bicubic", antialias=True,
                                          align_corners=False)[0]
    return float((got.to(torch.float64) - halve(x.to(torch.float64))).abs().max())


def turned(x, dec):
    """steps 3 - 5 alone"""
    r, h, v = (bool(d) for d in dec)
    if r:
        x = x.transpose(1, 2).flip(1)
    if h:
        x = x.flip(2)
    return x.flip(1) if v else x
