"""fp64 restatements of the evaluation metrics (ssl4gie_amd/metrics.py, csrc/metric_ops.hip) and the case generators of
tests/test_metrics_cpu.py and tests/test_gpu_metrics.py.  Not collected.  Everything here runs on the CPU and is
independent of the package: it is what the device results are held against."""
import numpy as np
import torch
import torch.nn.functional as F

EPS32 = float(np.finfo(np.float32).eps)


def ulp32(x):
    """spacing of fp32 at |x|"""
    return float(np.spacing(np.float32(abs(float(x)))))


def push_out(x, eps=1e-3):
    """logits nearer to zero than eps go to +-eps: the reference's own fp32 predicate sigmoid(x) > 0.5 is then x > 0"""
    return torch.where(x.abs() < eps, torch.where(x < 0, -eps, eps).to(x.dtype), x)


# ------------------------------------------------------------------ segmentation
def seg_counts64(logits, target, sigmoid=True):
    """logits [B, Hin, Win], target [B, H, W] (any dtype) -> (int64 [B, 3] counts, the fp64 map that was thresholded).
    The resize is F.interpolate(bilinear, align_corners=False) in fp64."""
    v = logits.double()
    if tuple(v.shape[1:]) != tuple(target.shape[1:]):
        v = F.interpolate(v.unsqueeze(1), size=tuple(target.shape[1:]), mode="bilinear", align_corners=False)[:, 0]
    m1 = (torch.sigmoid(v) > 0.5) if sigmoid else (v > 0.5)
    m2 = target.double() > 0.5
    B = v.shape[0]
    counts = torch.stack([m1.reshape(B, -1).sum(1), m2.reshape(B, -1).sum(1), (m1 & m2).reshape(B, -1).sum(1)], 1)
    return counts, v


def seg_scores32(counts, smooth):
    """the reference's four formulas (Binary_segmentation/Metrics/performance.py) on int64 counts [B, 3], evaluated as
    it evaluates them: int64 tensor + Python float -> fp32.  Returns per-image fp32 [4, B]."""
    m1, m2, inter = counts[:, 0], counts[:, 1], counts[:, 2]
    dice = 2.0 * (inter + smooth) / (m1 + m2 + smooth)
    iou = (inter + smooth) / (m1 + m2 - inter + smooth)
    prec = (inter + smooth) / (m1 + smooth)
    rec = (inter + smooth) / (m2 + smooth)
    out = torch.stack([dice, iou, prec, rec])
    assert out.dtype == torch.float32
    return out


def seg_case(B, H, W, seed, special=True):
    """fp32 logits [B, H, W] (3 randn, pushed out of +-1e-3) and a 0/1 fp32 target; with B >= 3 image 0 is the
    empty/empty one (all-negative logits, empty target) and image 1 is all-positive"""
    g = torch.Generator().manual_seed(seed)
    logits = push_out(3.0 * torch.randn(B, H, W, generator=g))
    target = (torch.rand(B, H, W, generator=g) < 0.4).float()
    if special and B >= 3:
        logits[0] = -logits[0].abs()
        target[0] = 0
        logits[1] = logits[1].abs()
    return logits, target


# ------------------------------------------------------------------ classification
def confusion64(preds, targets, C):
    """int64 [C, C] (row = target, column = prediction) and the number of rejected samples"""
    ok = (targets >= 0) & (targets < C) & (preds >= 0) & (preds < C)
    conf = torch.bincount(targets[ok] * C + preds[ok], minlength=C * C).view(C, C)
    return conf, int((~ok).sum())


def class_terms32(conf, smooth):
    """per-class fp32 terms [3, C] of the reference's loops (Classification/Metrics/performance.py), from the matrix"""
    tp, m1, m2 = conf.diagonal(), conf.sum(0), conf.sum(1)
    out = torch.stack([2.0 * (tp + smooth) / (m1 + m2 + smooth), (tp + smooth) / (m1 + smooth),
                       (tp + smooth) / (m2 + smooth)])
    assert out.dtype == torch.float32
    return out


def class_loop32(preds, targets, C, smooth):
    """the reference's loops themselves (restated), fp32 scalars: mean F1, mean precision, mean recall"""
    f1 = pr = rc = 0
    for i in range(C):
        m1, m2 = preds == i, targets == i
        inter = m1 * m2
        f1 += 2.0 * (inter.sum() + smooth) / (m1.sum() + m2.sum() + smooth)
        pr += (inter.sum() + smooth) / (m1.sum() + smooth)
        rc += (inter.sum() + smooth) / (m2.sum() + smooth)
    return torch.stack([f1 / C, pr / C, rc / C])


def class_case(B, C, seed, dtype=torch.float32):
    """logits [B, C] on a half-integer grid (ties are frequent), targets that never use the last class"""
    g = torch.Generator().manual_seed(seed)
    logits = (torch.randn(B, C, generator=g) * 2).round() / 2
    targets = torch.randint(0, max(C - 1, 1), (B,), generator=g)
    return logits.to(dtype), targets


# ------------------------------------------------------------------ median
MEDIAN_NS = (1, 2, 3, 10, 255, 256, 257, 65537)
MEDIAN_KINDS = ("random", "all_equal", "top16", "zeros_denormals", "one_inf", "duplicates", "sorted", "reversed")


def median_case(kind, n, seed=0):
    g = torch.Generator().manual_seed(seed + n)
    x = torch.rand(n, generator=g) * 4
    if kind == "all_equal":
        x = torch.full((n,), 0.7310585975646973)
    elif kind == "top16":  # the same sign, exponent and upper mantissa bits: only the last pass tells them apart
        bits = torch.randint(0, 1 << 16, (n,), generator=g, dtype=torch.int32) | (0x3FC5 << 16)
        x = bits.view(torch.float32)
    elif kind == "zeros_denormals":
        bits = torch.randint(0, 1 << 20, (n,), generator=g, dtype=torch.int32)
        x = torch.where(torch.rand(n, generator=g) < 0.5, torch.zeros(n), bits.view(torch.float32))
    elif kind == "one_inf":
        x[n // 2] = float("inf")
    elif kind == "duplicates":
        med = torch.median(x)
        x = torch.where(torch.rand(n, generator=g) < 0.6, med, x)
    elif kind == "sorted":
        x = torch.sort(x).values
    elif kind == "reversed":
        x = torch.sort(x, descending=True).values
    return x.contiguous()


# ------------------------------------------------------------------ depth
DEPTH_SHAPES = ((16, 23, 29), (16, 24, 29), (16, 29, 22), (16, 16, 16), (224, 270, 337))
SCALE_ = 10.0


def crop_offset(big, small):
    return int(round((big - small) / 2.0))  # torchvision's centre crop; Python rounds a half to even


def depth_case(S, H, W, seed):
    """pred, target [B, S, S], target_og [B, H, W]; B = 4 at S = 16 (a plain image, one with a fully masked band, one
    without a valid pixel, one with a constant prediction), B = 1 at S = 224.  25 % of the targets are zero."""
    g = torch.Generator().manual_seed(seed)
    B = 4 if S <= 32 else 1
    og = 0.05 + 0.9 * torch.rand(B, 1, H, W, generator=g)
    og = F.avg_pool2d(F.pad(og, (2, 2, 2, 2), mode="replicate"), 5, stride=1)          # a smooth depth map
    target = F.interpolate(og, size=(S, S), mode="bilinear", align_corners=False)[:, 0]
    pred = (target - 0.1) / 0.8 + 0.02 * torch.randn(B, S, S, generator=g)
    og = og[:, 0].clone()
    og[torch.rand(B, H, W, generator=g) < 0.25] = 0
    target = target.clone()
    target[torch.rand(B, S, S, generator=g) < 0.25] = 0
    if B == 4:
        og[1, H // 3: H // 2] = 0
        target[1, S // 3: S // 2] = 0
        og[2] = 0
        pred[3] = 0.5   # sums of 0.5 and 0.25 are exact in every precision and order: det == 0 exactly
    return pred.contiguous(), target.contiguous(), og.contiguous()


def depth_errors64(pred, target, target_og, scale_):
    """eval_depth.py:43-61 per image in fp64 -> float64 [B, 3] (rmse, lower-median relative error, mean absolute
    error); NaN where no pixel is valid"""
    p, t, og = pred.double(), target.double(), target_og.double()
    m = (t > 0).double()
    a00, a01, a11 = (m * p * p).sum((1, 2)), (m * p).sum((1, 2)), m.sum((1, 2))
    b0, b1 = (m * p * t).sum((1, 2)), (m * t).sum((1, 2))
    det = a00 * a11 - a01 * a01
    ok = det != 0
    safe = torch.where(ok, det, torch.ones_like(det))
    sc = torch.where(ok, (a11 * b0 - a01 * b1) / safe, torch.zeros_like(det))
    sh = torch.where(ok, (-a01 * b0 + a00 * b1) / safe, torch.zeros_like(det))
    out = sc.view(-1, 1, 1) * p + sh.view(-1, 1, 1)
    H, W = og.shape[1:]
    M = max(H, W)
    out = F.interpolate(out.unsqueeze(1), size=(M, M), mode="bilinear", align_corners=False)[:, 0]
    top, left = crop_offset(M, H), crop_offset(M, W)
    out = out[:, top:top + H, left:left + W].clamp(0.0, 1.0)
    out = torch.where(og == 0, torch.zeros_like(out), out) * scale_
    tg = og * scale_
    res = torch.full((p.shape[0], 3), float("nan"), dtype=torch.float64)
    for b in range(p.shape[0]):
        v = tg[b] > 0
        if v.any():
            d = (out[b] - tg[b])[v]
            res[b, 0] = torch.sqrt((d ** 2).mean())
            res[b, 1] = torch.median((d / tg[b][v]).abs())
            res[b, 2] = d.abs().mean()
    return res


def rel_dev(a, b):
    """|a - b| / |b| elementwise over the finite entries of b (float64), as a float64 tensor with 0 elsewhere; the NaN
    pattern of a and b must agree"""
    a, b = a.double(), b.double()
    assert torch.equal(torch.isnan(a), torch.isnan(b)), (a, b)
    fin = ~torch.isnan(b)
    out = torch.zeros_like(b)
    out[fin] = (a[fin] - b[fin]).abs() / b[fin].abs()
    return out
