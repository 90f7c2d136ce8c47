"""fp64 / plain-Python restatements of the linear-probe pieces, shared by test_probe_cpu.py and test_gpu_probe.py:
the rank rule and cross-entropy of ssl4gie_topk_update, the one-draw crop box of Models/mae/util/crop.py as a Python
loop over `math`, torch.optim.SGD's update, LARS's update and the BatchNorm head.  Nothing is read from any other tree;
every function takes and returns CPU tensors (or Python numbers)."""
import math

import numpy as np
import torch


# ---------------------------------------------------------------------------------------------- top-k scoring
def _above(a, b, ia, ib):
    """whether column ia (value a) is ordered above column ib (value b): a NaN above every number, equal values (and
    NaNs among themselves) by lower index first"""
    an, bn = a != a, b != b
    if an or bn:
        return (an and not bn) or (an and bn and ia < ib)
    return a > b or (a == b and ia < ib)


def ranks(logits, target):
    """Python loop: rank[i] = number of columns ordered above the target's logit; -1 for a target outside [0, C)"""
    x = logits.double().tolist()
    out = []
    for row, t in zip(x, target.tolist()):
        if not 0 <= t < len(row):
            out.append(-1)
            continue
        out.append(sum(1 for c, a in enumerate(row) if c != t and _above(a, row[t], c, t)))
    return torch.tensor(out, dtype=torch.int64)


def row_losses(logits, target):
    """fp64 cross-entropy per row (0 for a rejected row), logsumexp with the maximum subtracted; NaN rows stay NaN"""
    x = logits.double()
    C = x.shape[1]
    ok = (target >= 0) & (target < C)
    t = target.clamp(0, C - 1)
    lse = torch.logsumexp(x, dim=1)
    xt = x.gather(1, t.view(-1, 1))[:, 0]
    return torch.where(ok, lse - xt, torch.zeros_like(lse))


def topk_counts(rank, topk):
    """[hits per k ..., rows counted, rows rejected]"""
    ok = rank >= 0
    return [int((ok & (rank < k)).sum()) for k in topk] + [int(ok.sum()), int((~ok).sum())]


def tree_sum_rows(v):
    """the fixed order of ssl4gie_topk_update's loss sum, in fp64: thread t of 256 adds rows t, t + 256, ... in index
    order, then a halving tree over the 256 partials"""
    v = [float(a) for a in v]
    part = [0.0] * 256
    for t in range(256):
        for r in range(t, len(v), 256):
            part[t] += v[r]
    o = 128
    while o > 0:
        for t in range(o):
            part[t] += part[t + o]
        o >>= 1
    return part[0]


def permutation_rows(B, C, seed):
    """[B, C] fp32 rows, each a permutation of C distinct values: tie-free by construction"""
    g = torch.Generator().manual_seed(seed)
    vals = torch.linspace(-3.0, 3.0, C)
    return torch.stack([vals[torch.randperm(C, generator=g)] for _ in range(B)])


# ---------------------------------------------------------------------------------------------- crop boxes
def _round_half_even(v):
    return int(round(v))  # Python's round(): half to even


def tf_box(u, Hs, Ws, scale, ratio):
    """Models/mae/util/crop.py:23-42 for ONE image as a function of the four uniforms (area, log-aspect, top, left):
    -> ((top, left, h, w), (w_pre, h_pre)) with the sides before rounding.  log(ratio) and exp are fp32."""
    area = Hs * Ws
    target_area = area * (scale[0] + u[0] * (scale[1] - scale[0]))
    l0, l1 = float(np.log(np.float32(ratio[0]))), float(np.log(np.float32(ratio[1])))
    aspect = float(np.exp(np.float32(l0 + u[1] * (l1 - l0))))
    w_pre, h_pre = math.sqrt(target_area * aspect), math.sqrt(target_area / aspect)
    w = max(1, min(_round_half_even(w_pre), Ws))
    h = max(1, min(_round_half_even(h_pre), Hs))
    i = min(int(math.floor(u[2] * (Hs - h + 1))), Hs - h)
    j = min(int(math.floor(u[3] * (Ws - w + 1))), Ws - w)
    return (i, j, h, w), (w_pre, h_pre)


CROP_SIZES = ((256, 256), (224, 224), (37, 53))


def crop_uniforms():
    """the uniforms the crop tests share, on the CPU and on the device"""
    return torch.rand(4096, 4, dtype=torch.float64, generator=torch.Generator().manual_seed(0))


def tf_boxes(u, Hs, Ws, scale=(0.08, 1.0), ratio=(3.0 / 4.0, 4.0 / 3.0)):
    """-> (int32 [B, 4] boxes, the smallest distance of any pre-rounding side to a half-integer)"""
    boxes, margin = [], 1.0
    for row in u.tolist():
        b, pre = tf_box(row, Hs, Ws, scale, ratio)
        boxes.append(b)
        for v in pre:
            margin = min(margin, abs(v - math.floor(v) - 0.5))
    return torch.tensor(boxes, dtype=torch.int32), margin


# ---------------------------------------------------------------------------------------------- optimizers
def sgd_step(p, g, buf, lr, momentum, wd):
    """torch.optim.SGD, dampening 0, no Nesterov, with a zero-initialised buffer: -> (p, buf)"""
    d = g + wd * p
    buf = momentum * buf + d
    return p - lr * buf, buf


def lars_step(p, g, mu, lr, wd, momentum, trust):
    """Models/mae/util/lars.py:24-47 for one parameter: -> (p, mu)"""
    dp = g
    if p.ndim > 1:
        dp = dp + wd * p
        pn, un = p.norm(), dp.norm()
        q = trust * pn / un if (pn > 0 and un > 0) else torch.ones_like(pn)
        dp = dp * q
    mu = momentum * mu + dp
    return p - lr * mu, mu


# ---------------------------------------------------------------------------------------------- the BatchNorm head
def bn_head_train(x, w, b, running_mean, running_var, eps=1e-6, momentum=0.1):
    """Sequential(BatchNorm1d(affine=False, eps), Linear) in training mode: -> (logits, new running_mean,
    new running_var).  Batch statistics with the biased variance; the running variance takes the unbiased one."""
    n = x.shape[0]
    mean = x.mean(0)
    var = x.var(0, unbiased=False)
    xh = (x - mean) / torch.sqrt(var + eps)
    rm = (1 - momentum) * running_mean + momentum * mean
    rv = (1 - momentum) * running_var + momentum * var * n / (n - 1)
    return xh @ w.t() + b, rm, rv


def bn_head_eval(x, w, b, running_mean, running_var, eps=1e-6):
    return ((x - running_mean) / torch.sqrt(running_var + eps)) @ w.t() + b


def ce_head_grads(logits, target, xh):
    """mean cross-entropy over the rows and its gradients w.r.t. the Linear's weight and bias (xh = its input)"""
    n = logits.shape[0]
    p = torch.softmax(logits, dim=1)
    loss = (torch.logsumexp(logits, dim=1) - logits.gather(1, target.view(-1, 1))[:, 0]).mean()
    d = p.clone()
    d[torch.arange(n), target] -= 1.0
    d = d / n
    return loss, d.t() @ xh, d.sum(0)


def probe_head_curve(x, target, w, b, lr, wd, momentum, trust, eps=1e-6):
    """the G22 run restated: per step (loss, weight, bias, running_mean, running_var, logits) of the BatchNorm head under
    CrossEntropyLoss and LARS, in the dtype of the inputs (loss and logits before the step, the rest after it)"""
    D = x.shape[-1]
    rm, rv = torch.zeros(D, dtype=x.dtype), torch.ones(D, dtype=x.dtype)
    mw, mb = torch.zeros_like(w), torch.zeros_like(b)
    out = []
    for s in range(x.shape[0]):
        xs = x[s]
        mean, var = xs.mean(0), xs.var(0, unbiased=False)
        xh = (xs - mean) / torch.sqrt(var + eps)
        logits, rm, rv = bn_head_train(xs, w, b, rm, rv, eps)
        loss, gw, gb = ce_head_grads(logits, target[s], xh)
        w, mw = lars_step(w, gw, mw, lr, wd, momentum, trust)
        b, mb = lars_step(b, gb, mb, lr, wd, momentum, trust)
        out.append((loss, w, b, rm, rv, logits))
    return out
