"""Not a test: numpy restatements of the rules of include/ssl4gie_hip.h's RandAugment / RandomErasing section, the
integer noise stream, and the fixed cases that tests/test_randaug_checks_cpu.py (against PIL) and
tests/test_gpu_randaug.py (against the kernels) share.

Images are uint8 [S, S, 3].  Every pixel rule is PIL's (ImageOps, ImageEnhance, Image.transform / rotate with
BICUBIC); the CPU tests hold each restatement here to PIL bit for bit, the GPU tests hold the kernels to the
restatements bit for bit, so the kernels are PIL's rules by transitivity and the GPU tests need no PIL."""
import math

import numpy as np

N_OPS = 15
(AUTO_CONTRAST, EQUALIZE, INVERT, ROTATE, POSTERIZE, SOLARIZE, SOLARIZE_ADD, COLOR, CONTRAST, BRIGHTNESS, SHARPNESS,
 SHEAR_X, SHEAR_Y, TRANSLATE_X, TRANSLATE_Y) = range(N_OPS)
SKIP = 255
GEOMETRIC = (ROTATE, SHEAR_X, SHEAR_Y, TRANSLATE_X, TRANSLATE_Y)
FILL = (124, 116, 104)   # tuple(min(255, round(255 m)) for m in the ImageNet mean)
IDENTITY = (1.0, 0.0, 0.0, 0.0, 1.0, 0.0)
IMAGENET_MEAN, IMAGENET_STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


# ------------------------------------------------------------------------------------------------ pixel rules
def lum(img):
    """PIL's RGB -> L"""
    r, g, b = (img[..., c].astype(np.int64) for c in range(3))
    return ((19595 * r + 38470 * g + 7471 * b + 0x8000) >> 16).astype(np.uint8)


def hist(ch):
    return np.bincount(np.asarray(ch, np.uint8).reshape(-1), minlength=256).astype(np.int64)


def blend(d, v, f):
    """Image.blend(degenerate, image, f) on arrays: fp32, the product and the sum rounded one by one"""
    f = np.float32(f)
    d32, v32 = np.asarray(d, np.float32), np.asarray(v, np.float32)
    t = d32 + f * (v32 - d32)
    with np.errstate(invalid="ignore"):
        return np.where(t <= 0, 0, np.where(t >= 255, 255, t.astype(np.int64))).astype(np.uint8)


_IDENT = np.arange(256, dtype=np.uint8)


def lut_autocontrast(h):
    nz = np.nonzero(h)[0]
    if len(nz) == 0 or nz[-1] <= nz[0]:
        return _IDENT.copy()
    lo, hi = int(nz[0]), int(nz[-1])
    s = 255.0 / (hi - lo)
    o = -lo * s
    return np.array([min(255, max(0, int(i * s + o))) for i in range(256)], dtype=np.uint8)


def equalize_step(h):
    """None when the channel holds at most one level, else ImageOps.equalize's step (0: identity)"""
    nz = [int(v) for v in h if v]
    if len(nz) <= 1:
        return None
    return (sum(nz) - nz[-1]) // 255


def lut_equalize(h):
    step = equalize_step(h)
    if not step:
        return _IDENT.copy()
    lut, n = [], step // 2
    for i in range(256):
        lut.append(min(255, n // step))
        n += int(h[i])
    return np.array(lut, dtype=np.uint8)


def lut_posterize(bits):
    bits = int(bits)
    if bits >= 8:
        return _IDENT.copy()
    return (_IDENT & np.uint8(~(2 ** (8 - bits) - 1) & 0xff)).astype(np.uint8)


def lut_solarize(thresh):
    i = np.arange(256)
    return np.where(i < int(thresh), i, 255 - i).astype(np.uint8)


def lut_solarize_add(add):
    i = np.arange(256)
    return np.where(i < 128, np.minimum(255, i + int(add)), i).astype(np.uint8)


def contrast_mean(h_l):
    """int(mean of L + 0.5), the mean from the histogram as ImageStat takes it"""
    return int(float(sum(i * int(h_l[i]) for i in range(256))) / float(int(h_l.sum())) + 0.5)


def smooth(img):
    """ImageFilter.SMOOTH: interior pixels (1 1 1 / 1 5 1 / 1 1 1) / 13 — the fp32 coefficients 1 / 13 and 5 / 13,
    the sum started at 0.5, rows taken from the one below upwards, three products per row added left to right, every
    operation rounded to fp32 — clipped and truncated; the one-pixel border is the source"""
    S = img.shape[0]
    k1, k5 = np.float32(1.0) / np.float32(13.0), np.float32(5.0) / np.float32(13.0)
    out = img.copy()
    if S < 3:
        return out
    v = img.astype(np.float32)
    c = slice(1, S - 1)
    row = lambda r, km: (v[r, 0:S - 2] * k1 + v[r, 1:S - 1] * km) + v[r, 2:S] * k1
    ss = np.float32(0.5) + row(slice(2, S), k1)
    ss = ss + row(slice(1, S - 1), k5)
    ss = ss + row(slice(0, S - 2), k1)
    out[c, c] = np.where(ss <= 0, 0, np.where(ss >= 255, 255, ss.astype(np.int64))).astype(np.uint8)
    return out


def _cubic(v1, v2, v3, v4, d):
    p1 = v2
    p2 = -v1 + v3
    p3 = 2 * (v1 - v2) + v3 - v4
    p4 = -v1 + v2 - v3 + v4
    return p1 + d * (p2 + d * (p3 + d * p4))


def affine(img, m, fill=FILL):
    """Image.transform(size, AFFINE, m, BICUBIC, fillcolor=fill), all fp64"""
    S = img.shape[0]
    m = [np.float64(v) for v in m]
    ys, xs = np.mgrid[0:S, 0:S]
    xc, yc = xs + 0.5, ys + 0.5
    with np.errstate(invalid="ignore", over="ignore"):
        xin = m[0] * xc + m[1] * yc + m[2]
        yin = m[3] * xc + m[4] * yc + m[5]
        inside = (xin >= 0) & (xin < S) & (yin >= 0) & (yin < S)   # NaN: not inside
    xin = np.where(inside, xin, 0.5) - 0.5
    yin = np.where(inside, yin, 0.5) - 0.5
    x0, y0 = np.floor(xin), np.floor(yin)
    dx, dy = xin - x0, yin - y0
    x0, y0 = x0.astype(np.int64), y0.astype(np.int64)
    v = img.astype(np.float64)
    rows = []
    for j in range(4):
        yi = np.clip(y0 - 1 + j, 0, S - 1)
        taps = [v[yi, np.clip(x0 - 1 + k, 0, S - 1)] for k in range(4)]
        rows.append(_cubic(*taps, dx[..., None]))
    r = _cubic(*rows, dy[..., None])
    q = np.where(r <= 0, 0, np.where(r >= 255, 255, r.astype(np.int64))).astype(np.uint8)
    return np.where(inside[..., None], q, np.array(fill, dtype=np.uint8))


def rotate_matrix(deg, S, rounded=False):
    """Image.rotate's matrix about (S / 2, S / 2); rounded=True rounds cos and sin to 15 decimals as PIL does (the
    engine's draw does not)"""
    a = -math.radians(deg)
    rnd = (lambda v: round(v, 15)) if rounded else (lambda v: v)
    m = [rnd(math.cos(a)), rnd(math.sin(a)), 0.0, rnd(-math.sin(a)), rnd(math.cos(a)), 0.0]
    cx = cy = S / 2.0
    m[2] = m[0] * -cx + m[1] * -cy + m[2]
    m[5] = m[3] * -cx + m[4] * -cy + m[5]
    m[2] += cx
    m[5] += cy
    return tuple(m)


def op_matrix(op, arg, S):
    """the AFFINE coefficients of a geometric op with argument arg (degrees, shear, or pixels)"""
    arg = float(arg)
    if op == ROTATE:
        return rotate_matrix(arg, S)
    if op == SHEAR_X:
        return (1.0, arg, 0.0, 0.0, 1.0, 0.0)
    if op == SHEAR_Y:
        return (1.0, 0.0, 0.0, arg, 1.0, 0.0)
    if op == TRANSLATE_X:
        return (1.0, 0.0, arg, 0.0, 1.0, 0.0)
    if op == TRANSLATE_Y:
        return (1.0, 0.0, 0.0, 0.0, 1.0, arg)
    return IDENTITY


def apply_lut(img, luts):
    out = np.empty_like(img)
    for c in range(3):
        out[..., c] = luts[c][img[..., c]]
    return out


def apply_op(img, op, arg=0.0, matrix=IDENTITY, fill=FILL):
    """one op of the table on one image; arg as the kernel takes it (fp32): bits, threshold, addend, factor"""
    op = int(op)
    arg = np.float32(arg)
    if op in (AUTO_CONTRAST, EQUALIZE):
        f = lut_autocontrast if op == AUTO_CONTRAST else lut_equalize
        return apply_lut(img, [f(hist(img[..., c])) for c in range(3)])
    if op == INVERT:
        return (255 - img).astype(np.uint8)
    if op == POSTERIZE:
        return apply_lut(img, [lut_posterize(int(arg))] * 3)
    if op == SOLARIZE:
        return apply_lut(img, [lut_solarize(int(arg))] * 3)
    if op == SOLARIZE_ADD:
        return apply_lut(img, [lut_solarize_add(int(arg))] * 3)
    if op == COLOR:
        return blend(lum(img)[..., None], img, arg)
    if op == CONTRAST:
        return blend(contrast_mean(hist(lum(img))), img, arg)
    if op == BRIGHTNESS:
        return blend(0, img, arg)
    if op == SHARPNESS:
        return blend(smooth(img), img, arg)
    if op in GEOMETRIC:
        return affine(img, matrix, fill)
    return img.copy()


def layer_ref(imgs, op, arg, matrix, fill=FILL):
    """ssl4gie_randaug_layer on uint8 [B, S, S, 3]"""
    return np.stack([apply_op(imgs[b], op[b], arg[b], matrix[b], fill) for b in range(imgs.shape[0])])


def quantize_ref(x):
    """ssl4gie_quantize_u8: fp32 [B, 3, S, S] in 0..255 units -> uint8 [B, S, S, 3]; clamp, + 0.5, truncate"""
    x = np.asarray(x, np.float32)
    with np.errstate(invalid="ignore"):
        c = np.where(x >= 0, np.minimum(x, np.float32(255.0)), np.float32(0.0)).astype(np.float32)   # NaN -> 0
    return np.ascontiguousarray((c + np.float32(0.5)).astype(np.int64).astype(np.uint8).transpose(0, 2, 3, 1))


# ------------------------------------------------------------------------------------------------ timm's level maps
def timm_level_arg(op, magnitude, negate, inc, S):
    """a literal scalar transcription of timm 0.3.2's level functions (auto_augment.py, _MAX_LEVEL = 10): the argument
    of op at `magnitude`, `negate` standing for `random.random() > 0.5` of _randomly_negate.  None: no argument"""
    neg = lambda v: -v if negate else v
    level = magnitude
    if op in (AUTO_CONTRAST, EQUALIZE, INVERT):
        return None
    if op == ROTATE:
        return neg((level / 10) * 30.)
    if op == POSTERIZE:
        return 4 - int((level / 10) * 4) if inc else int((level / 10) * 4)
    if op == SOLARIZE:
        return 256 - int((level / 10) * 256) if inc else int((level / 10) * 256)
    if op == SOLARIZE_ADD:
        return int((level / 10) * 110)
    if op in (COLOR, CONTRAST, BRIGHTNESS, SHARPNESS):
        return 1.0 + neg((level / 10) * .9) if inc else (level / 10) * 1.8 + 0.1
    if op in (SHEAR_X, SHEAR_Y):
        return neg((level / 10) * 0.3)
    if op in (TRANSLATE_X, TRANSLATE_Y):
        return neg((level / 10) * 0.45) * S
    raise ValueError(op)


# ------------------------------------------------------------------------------------------------ RandomErasing
def erase_boxes_loop(u, H, W, probability=0.25, min_area=0.02, max_area=1 / 3, min_aspect=0.3):
    """timm's RandomErasing._erase box choice (max_count = 1) as a literal loop over uniforms u [B, 41]: u[b, 0] the
    apply draw, then per attempt (area, log-aspect, top, left).  int32 [B, 4] = (top, left, h, w), zeros: no erase"""
    u = np.asarray(u, np.float64)
    out = np.zeros((u.shape[0], 4), dtype=np.int32)
    l0, l1 = math.log(min_aspect), math.log(1 / min_aspect)
    for b in range(u.shape[0]):
        if u[b, 0] > probability:
            continue
        area = H * W
        for attempt in range(10):
            ua, ur, ut, ul = u[b, 1 + 4 * attempt:5 + 4 * attempt]
            target_area = (min_area + (max_area - min_area) * ua) * area
            aspect_ratio = math.exp(l0 + (l1 - l0) * ur)
            h = int(round(math.sqrt(target_area * aspect_ratio)))
            w = int(round(math.sqrt(target_area / aspect_ratio)))
            if w < W and h < H:
                top = min(int(math.floor(ut * (H - h + 1))), H - h)     # random.randint(0, H - h)
                left = min(int(math.floor(ul * (W - w + 1))), W - w)
                out[b] = (top, left, h, w)
                break
    return out


# ------------------------------------------------------------------------------------------------ the noise stream
_M0, _M1, _W0, _W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
_MASK = np.uint64(0xffffffff)


def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """Philox4x32-10 (Salmon et al. 2011) on uint64 arrays holding 32-bit words: the four output words"""
    c0, c1, c2, c3 = (np.asarray(c, np.uint64) & _MASK for c in (c0, c1, c2, c3))
    k0, k1 = np.uint64(k0 & 0xffffffff), np.uint64(k1 & 0xffffffff)
    for r in range(10):
        p0, p1 = np.uint64(_M0) * c0, np.uint64(_M1) * c2
        c0, c1, c2, c3 = ((p1 >> np.uint64(32)) ^ c1 ^ k0, p1 & _MASK, (p0 >> np.uint64(32)) ^ c3 ^ k1, p0 & _MASK)
        k0, k1 = (k0 + np.uint64(_W0)) & _MASK, (k1 + np.uint64(_W1)) & _MASK
    return c0, c1, c2, c3


def noise_ints(seed, b, c, y, x):
    """the two 24-bit integers of element (b, c, y, x): counter (x, y, c, b), key (seed low, seed high); the top 24
    bits of output words 0 and 1"""
    w0, w1, _, _ = philox4x32_10(x, y, c, b, int(seed) & 0xffffffff, (int(seed) >> 32) & 0xffffffff)
    return (w0 >> np.uint64(8)).astype(np.int64), (w1 >> np.uint64(8)).astype(np.int64)


def noise_from_ints(k1, k2, dtype):
    """Box-Muller on u = (k + 1) 2^-24: sqrt(-2 ln u1) cos(2 pi u2), every operation in `dtype`"""
    t = np.dtype(dtype).type
    u1 = (k1 + 1).astype(dtype) * t(2.0 ** -24)
    u2 = (k2 + 1).astype(dtype) * t(2.0 ** -24)
    return np.sqrt(t(-2.0) * np.log(u1)) * np.cos(t(2.0 * math.pi) * u2)


def noise_field(seed, B, S, dtype, rand_mode=False):
    """[B, 3, S, S] noise of the pixel mode, or [B, 3, 1, 1] of the rand mode (key (seed, b, c, 0, 0))"""
    if rand_mode:
        b, c = np.mgrid[0:B, 0:3]
        k1, k2 = noise_ints(seed, b, c, 0 * b, 0 * b)
        return noise_from_ints(k1, k2, dtype)[:, :, None, None]
    b, c, y, x = np.mgrid[0:B, 0:3, 0:S, 0:S]
    return noise_from_ints(*noise_ints(seed, b, c, y, x), dtype)


def box_mask(box, S):
    """bool [B, 1, S, S]: inside box[b] = (top, left, h, w)"""
    box = np.asarray(box, np.int64)
    y, x = np.mgrid[0:S, 0:S]
    t, l, h, w = (box[:, i, None, None] for i in range(4))
    return ((y >= t) & (y < t + h) & (x >= l) & (x < l + w) & (h > 0) & (w > 0))[:, None]


# ------------------------------------------------------------------------------------------------ the fixed cases
def image(S, seed, kind="noise"):
    """uint8 [S, S, 3]"""
    rs = np.random.RandomState(1000 * S + seed)
    if kind == "noise":
        return rs.randint(0, 256, size=(S, S, 3)).astype(np.uint8)
    if kind == "smooth":   # a low-frequency image with a narrow range: AutoContrast and Equalize have work to do
        y, x = np.mgrid[0:S, 0:S] / float(S)
        ch = [60 + 90 * np.sin(3 * x + c) * np.cos(2 * y - c) + rs.randint(0, 12, size=(S, S)) for c in range(3)]
        return np.clip(np.stack(ch, axis=2), 0, 255).astype(np.uint8)
    if kind == "const_channel":   # G constant: AutoContrast hi <= lo, Equalize with one bin
        img = rs.randint(0, 256, size=(S, S, 3)).astype(np.uint8)
        img[..., 1] = 77
        return img
    if kind == "step_zero":   # S = 16: 256 pixels, two of them in the last bin, so Equalize's step is 254 // 255 = 0
        assert S == 16
        img = rs.randint(0, 256, size=(256, 3)).astype(np.uint8)
        img[rs.permutation(256)[:2]] = 255
        return img.reshape(16, 16, 3)
    if kind == "step_one":   # ONE pixel in the last bin: step = (S S - 1) // 255, which is 1 at S = 16 and S = 20
        img = np.empty((S * S, 3), dtype=np.uint8)
        for c in range(3):
            col = rs.randint(0, 40, size=S * S).astype(np.uint8)   # 40 levels
            col[:S * S - 256] = 3                                  # all but 256 pixels on one level
            col[-1] = 250                                          # the last bin holds a single pixel
            img[:, c] = rs.permutation(col)
        return img.reshape(S, S, 3)
    if kind == "half_mean":   # L is 10 on one half and 11 on the other: its mean falls on 10.5
        img = np.full((S, S, 3), 10, dtype=np.uint8)
        img[:, S // 2:] = 11
        return img
    raise ValueError(kind)


FACTORS = (0.1, 1.0, 1.9, float(np.float32(0.7345678)))


def op_cases(S):
    """[(name, image kind, op, arg, matrix)]: every op id with the arguments the issue names; the branch cases only
    where they exist at this S"""
    cases = []
    kinds = ["noise", "smooth", "const_channel", "half_mean", "step_one"] + (["step_zero"] if S == 16 else [])
    for kind in kinds:
        cases += [(f"autocontrast/{kind}", kind, AUTO_CONTRAST, 0.0, IDENTITY),
                  (f"equalize/{kind}", kind, EQUALIZE, 0.0, IDENTITY)]
    cases.append(("invert", "noise", INVERT, 0.0, IDENTITY))
    for bits in (0, 1, 4, 8):
        cases.append((f"posterize/{bits}", "noise", POSTERIZE, float(bits), IDENTITY))
    for thresh in (0, 26, 128, 256):
        cases.append((f"solarize/{thresh}", "noise", SOLARIZE, float(thresh), IDENTITY))
    for add in (0, 99, 110):
        cases.append((f"solarize_add/{add}", "noise", SOLARIZE_ADD, float(add), IDENTITY))
    for op, name in ((COLOR, "color"), (CONTRAST, "contrast"), (BRIGHTNESS, "brightness"), (SHARPNESS, "sharpness")):
        for f in FACTORS:
            cases.append((f"{name}/{f:g}", "noise", op, f, IDENTITY))
    cases.append(("contrast/half_mean", "half_mean", CONTRAST, 1.9, IDENTITY))
    for deg in (30.0, -30.0, 7.3, 0.0):
        cases.append((f"rotate/{deg:g}", "smooth", ROTATE, deg, rotate_matrix(deg, S)))
    for s in (0.3, -0.3, 0.11):
        cases.append((f"shear_x/{s:g}", "noise", SHEAR_X, s, op_matrix(SHEAR_X, s, S)))
        cases.append((f"shear_y/{s:g}", "smooth", SHEAR_Y, s, op_matrix(SHEAR_Y, s, S)))
    for t in (3.0, -2.0, 0.45 * 0.9 * S, -1.37):   # whole-pixel and fractional
        cases.append((f"translate_x/{t:g}", "noise", TRANSLATE_X, t, op_matrix(TRANSLATE_X, t, S)))
        cases.append((f"translate_y/{t:g}", "smooth", TRANSLATE_Y, t, op_matrix(TRANSLATE_Y, t, S)))
    return cases


def layer_batch(S, cases=None):
    """the cases of op_cases(S) as one batch: imgs uint8 [B, S, S, 3], op uint8 [B], arg fp32 [B], matrix fp64 [B, 6]"""
    cases = op_cases(S) if cases is None else cases
    imgs = np.stack([image(S, i % 7, kind) for i, (_, kind, _, _, _) in enumerate(cases)])
    op = np.array([c[2] for c in cases], dtype=np.uint8)
    arg = np.array([c[3] for c in cases], dtype=np.float32)
    matrix = np.array([c[4] for c in cases], dtype=np.float64)
    return imgs, op, arg, matrix
