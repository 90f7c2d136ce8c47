"""Faster R-CNN heads on the MI355X engine: the class Object_detection/train_detection.py:244-250 constructs,

    FasterRCNN(backbone, num_classes, image_mean=..., image_std=..., **torchvision 0.10 keyword defaults)

with torchvision 0.10's state_dict keys (`backbone.*`, `rpn.head.{conv,cls_logits,bbox_pred}.*`,
`roi_heads.box_head.{fc6,fc7}.*`, `roi_heads.box_predictor.{cls_score,bbox_pred}.*`, no buffers).  torchvision is not
installed: every rule below is stated from torchvision 0.10's published source (models/detection/{faster_rcnn, rpn,
roi_heads, _utils, anchor_utils, transform}.py, ops/{boxes, roi_align, poolers}.py).

The parts torchvision runs as C++ / CUDA ops are HIP kernels (csrc/det_head_ops.hip, ops.nms_segments / rpn_decode /
roi_decode / roi_align_{fwd,bwd}); convolutions and GEMMs are the engine's nodes.  Everything between the kernels keeps
STATIC shapes so that `forward` never waits for the device: proposals are [B, post_nms_top_n, 4] with a validity flag,
the sampled RoIs of the training step are [B, batch_size_per_image] with one, the losses are masked sums.  The one
read-back is the detection counts that split the result list of `eval`.

SSL4GIE_FUSED_DET_HEADS=0 (and CPU tensors) select the torch formulations of the three kernels, kept in this file with
the kernels' signatures (`*_torch`): they are the tests' fp32 reference.
"""
from __future__ import annotations

import math
import os
from collections import OrderedDict

import torch
import torch.nn as nn
import torch.nn.functional as F_

from .. import ops
from ..engine import EngineModule, LinearFn
from ..dpt_engine import _write_grad

BBOX_XFORM_CLIP = math.log(1000.0 / 16)
ANCHOR_SIZES = (32, 64, 128, 256, 512)
ANCHOR_RATIOS = (0.5, 1.0, 2.0)
POOL = 7


def _fused(*ts):
    return all(t.is_cuda for t in ts) and os.environ.get("SSL4GIE_FUSED_DET_HEADS", "1") != "0"


# ------------------------------------------------------------------------------------------------
# torch formulations (fp32 reference of the kernels; CPU path; SSL4GIE_FUSED_DET_HEADS=0)
# ------------------------------------------------------------------------------------------------
def base_anchors(sizes=ANCHOR_SIZES, ratios=ANCHOR_RATIOS):
    """AnchorGenerator.generate_anchors per level: fp32 [L, A, 4] = round([-w, -h, w, h] / 2)"""
    out = []
    ar = torch.as_tensor(ratios, dtype=torch.float32)
    h_r = torch.sqrt(ar)
    w_r = 1 / h_r
    for s in sizes:
        scales = torch.as_tensor([s], dtype=torch.float32)
        ws = (w_r[:, None] * scales[None, :]).view(-1)
        hs = (h_r[:, None] * scales[None, :]).view(-1)
        out.append((torch.stack([-ws, -hs, ws, hs], dim=1) / 2).round())
    return torch.stack(out)


def grid_anchors(base, grids, F, device="cpu"):
    """AnchorGenerator.grid_anchors: a list of fp32 [g * g * A, 4], anchor index fastest within a location"""
    out = []
    for b, g in zip(base, grids):
        stride = F // g
        s = torch.arange(0, g, dtype=torch.float32, device=device) * stride
        sy, sx = torch.meshgrid(s, s, indexing="ij")
        sx, sy = sx.reshape(-1), sy.reshape(-1)
        shifts = torch.stack((sx, sy, sx, sy), dim=1)
        out.append((shifts.view(-1, 1, 4) + b.to(device).view(1, -1, 4)).reshape(-1, 4))
    return out


def box_iou(a, b):
    """torchvision.ops.box_iou: [len(a), len(b)]"""
    area_a = (a[:, 2] - a[:, 0]) * (a[:, 3] - a[:, 1])
    area_b = (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])
    lt = torch.max(a[:, None, :2], b[:, :2])
    rb = torch.min(a[:, None, 2:], b[:, 2:])
    wh = (rb - lt).clamp(min=0)
    inter = wh[:, :, 0] * wh[:, :, 1]
    return inter / (area_a[:, None] + area_b - inter)


def decode_boxes(ref, deltas, weights):
    """BoxCoder.decode_single for one delta set per reference box: ref [n, 4], deltas [n, 4]"""
    wx, wy, ww, wh = weights
    widths = ref[:, 2] - ref[:, 0]
    heights = ref[:, 3] - ref[:, 1]
    ctr_x = ref[:, 0] + 0.5 * widths
    ctr_y = ref[:, 1] + 0.5 * heights
    dx, dy = deltas[:, 0] / wx, deltas[:, 1] / wy
    dw, dh = deltas[:, 2] / ww, deltas[:, 3] / wh
    dw = torch.clamp(dw, max=BBOX_XFORM_CLIP)
    dh = torch.clamp(dh, max=BBOX_XFORM_CLIP)
    pcx = dx * widths + ctr_x
    pcy = dy * heights + ctr_y
    pw = torch.exp(dw) * widths
    ph = torch.exp(dh) * heights
    return torch.stack([pcx - 0.5 * pw, pcy - 0.5 * ph, pcx + 0.5 * pw, pcy + 0.5 * ph], dim=1)


def encode_boxes(gt, ref, weights):
    """BoxCoder.encode_single (torchvision's encode_boxes)"""
    wx, wy, ww, wh = weights
    ew, eh = ref[:, 2] - ref[:, 0], ref[:, 3] - ref[:, 1]
    ecx, ecy = ref[:, 0] + 0.5 * ew, ref[:, 1] + 0.5 * eh
    gw, gh = gt[:, 2] - gt[:, 0], gt[:, 3] - gt[:, 1]
    gcx, gcy = gt[:, 0] + 0.5 * gw, gt[:, 1] + 0.5 * gh
    return torch.stack([wx * (gcx - ecx) / ew, wy * (gcy - ecy) / eh, ww * torch.log(gw / ew), wh * torch.log(gh / eh)],
                       dim=1)


def _clip_and_flag(boxes, scores, W, H, min_size, score_thresh):
    x1 = boxes[:, 0].clamp(min=0, max=W)
    y1 = boxes[:, 1].clamp(min=0, max=H)
    x2 = boxes[:, 2].clamp(min=0, max=W)
    y2 = boxes[:, 3].clamp(min=0, max=H)
    valid = ((x2 - x1) >= min_size) & ((y2 - y1) >= min_size) & (scores >= score_thresh)
    return torch.stack([x1, y1, x2, y2], dim=1), valid.to(torch.uint8)


def rpn_decode_torch(heads, grids, k_off, base, topk_idx, F, min_size, score_thresh):
    """ops.rpn_decode in torch: the anchors of the whole level are built and gathered"""
    B, ktot = topk_idx.shape
    A = base.shape[1]
    dev = topk_idx.device
    anchors = grid_anchors(base, grids, F, dev)
    bo, so = [], []
    for l, (h, g) in enumerate(zip(heads, grids)):
        idx = topk_idx[:, k_off[l]:k_off[l + 1]]
        h = h.view(B, g * g, -1)
        logit = h[:, :, :A].reshape(B, -1).gather(1, idx)
        d = h[:, :, A:5 * A].reshape(B, g * g * A, 4).gather(1, idx[:, :, None].expand(-1, -1, 4))
        a = anchors[l][idx.reshape(-1)]
        bo.append(decode_boxes(a, d.reshape(-1, 4), (1.0, 1.0, 1.0, 1.0)).view(B, -1, 4))
        so.append(torch.sigmoid(logit))
    boxes, scores = torch.cat(bo, 1), torch.cat(so, 1)
    boxes, valid = _clip_and_flag(boxes.reshape(-1, 4), scores.reshape(-1), F, F, min_size, score_thresh)
    return boxes.view(B, ktot, 4), scores, valid.view(B, ktot)


def roi_decode_torch(proposals, logits, deltas, weights, W, H, min_size, score_thresh):
    """ops.roi_decode in torch"""
    K, Cn = logits.shape
    scores = F_.softmax(logits, -1)[:, 1:]
    ref = proposals[:, None, :].expand(K, Cn - 1, 4).reshape(-1, 4)
    boxes = decode_boxes(ref, deltas.reshape(K, Cn, 4)[:, 1:].reshape(-1, 4), weights)
    boxes, valid = _clip_and_flag(boxes, scores.reshape(-1), W, H, min_size, score_thresh)
    return boxes.view(K, Cn - 1, 4), scores.contiguous(), valid.view(K, Cn - 1)


def nms_segments_torch(boxes, seg_off, thr, valid=None, max_seg=None):
    """ops.nms_segments in torch: the IoU matrix of a segment in fp32 on the tensors' device, the greedy sweep on the
    host (as torchvision's CUDA nms does it)"""
    n = boxes.shape[0]
    so = seg_off.detach().cpu().tolist()
    keep_rank = torch.full((n,), -1, dtype=torch.int32)
    count = torch.zeros(len(so) - 1, dtype=torch.int32)
    for s in range(len(so) - 1):
        a, b = so[s], so[s + 1]
        if max_seg is not None:
            b = min(b, a + max_seg)
        if b - a > ops._lib.NMS_MAX_PER_SEGMENT:
            raise ValueError(f"nms_segments: {b - a} boxes in a segment, the cap is {ops._lib.NMS_MAX_PER_SEGMENT}")
        if b <= a:
            continue
        over = (box_iou(boxes[a:b], boxes[a:b]) > thr).cpu().numpy()
        removed = (~valid[a:b].bool()).cpu().numpy().copy() if valid is not None else \
            torch.zeros(b - a, dtype=torch.bool).numpy()
        r = 0
        for i in range(b - a):
            if removed[i]:
                continue
            keep_rank[a + i] = r
            r += 1
            removed[i + 1:] |= over[i, i + 1:]
        count[s] = r
    return keep_rank.to(boxes.device), count.to(boxes.device)


def roi_levels_torch(rois):
    """LevelMapper(2, 5): floor(4 + log2(sqrt(area) / 224) + 1e-6) clamped to [2, 5], minus 2"""
    s = torch.sqrt((rois[:, 2] - rois[:, 0]) * (rois[:, 3] - rois[:, 1]))
    lv = torch.floor(4 + torch.log2(s / 224) + torch.tensor(1e-6, dtype=s.dtype, device=s.device))
    return (torch.clamp(lv, min=2, max=5).to(torch.int64) - 2)


def _roi_align_level(m, scale, rois, bidx):
    """torchvision.ops.roi_align(m, rois, 7, scale, sampling_ratio=2, aligned=False) for NCHW m: [k, C, 7, 7]"""
    B, C, H, W = m.shape
    k = rois.shape[0]
    dt, dev = rois.dtype, rois.device
    sw, sh = rois[:, 0] * scale, rois[:, 1] * scale
    ew, eh = rois[:, 2] * scale, rois[:, 3] * scale
    bw = torch.clamp(ew - sw, min=1.0) / POOL
    bh = torch.clamp(eh - sh, min=1.0) / POOL
    p = torch.arange(POOL, dtype=dt, device=dev)
    i = torch.arange(2, dtype=dt, device=dev) + 0.5
    # [k, 7, 2] -> [k, 14]: bin-major, sample inside
    y = (sh[:, None, None] + p[None, :, None] * bh[:, None, None] + i[None, None, :] * bh[:, None, None] / 2).view(k, -1)
    x = (sw[:, None, None] + p[None, :, None] * bw[:, None, None] + i[None, None, :] * bw[:, None, None] / 2).view(k, -1)

    def axis(c, n):
        out = (c < -1.0) | (c > n)
        c = c.clamp(min=0)
        lo = c.floor().to(torch.int64)
        edge = lo >= n - 1
        lo = torch.where(edge, torch.full_like(lo, n - 1), lo)
        hi = torch.where(edge, lo, lo + 1)
        c = torch.where(edge, lo.to(dt), c)
        l = c - lo.to(dt)
        return out, lo.clamp(0, n - 1), hi.clamp(0, n - 1), l, 1.0 - l

    oy, yl, yh, ly, hy = axis(y, H)
    ox, xl, xh, lx, hx = axis(x, W)
    flat = m.permute(0, 2, 3, 1).reshape(B * H * W, C)
    base = (bidx.to(torch.int64) * H * W)[:, None, None]

    def tap(yy, xx, wy, wx):
        idx = base + yy[:, :, None] * W + xx[:, None, :]
        return flat[idx.reshape(-1)].view(k, 2 * POOL, 2 * POOL, C) * (wy[:, :, None] * wx[:, None, :])[..., None]

    v = tap(yl, xl, hy, hx) + tap(yl, xh, hy, lx) + tap(yh, xl, ly, hx) + tap(yh, xh, ly, lx)
    v = torch.where((oy[:, :, None] | ox[:, None, :])[..., None], torch.zeros((), dtype=v.dtype, device=dev), v)
    v = v.view(k, POOL, 2, POOL, 2, C).sum(dim=(2, 4)) / 4
    return v.permute(0, 3, 1, 2)


def roi_align_torch(maps, scales, rois, roi_batch, out_dtype=None, chunk=256):
    """ops.roi_align_fwd in torch, differentiable in the maps: [K, C * 49] in (c, ph, pw) order"""
    K, C = rois.shape[0], maps[0].shape[1]
    lv = roi_levels_torch(rois)
    out = torch.zeros(K, C, POOL, POOL, dtype=maps[0].dtype, device=rois.device)
    for l in range(4):
        idx = torch.nonzero(lv == l).view(-1)
        for s in range(0, idx.numel(), chunk):
            j = idx[s:s + chunk]
            out = out.index_put((j,), _roi_align_level(maps[l], scales[l], rois[j], roi_batch[j]))
    out = out.reshape(K, C * POOL * POOL)
    return out if out_dtype is None else out.to(out_dtype)


# ------------------------------------------------------------------------------------------------
# engine nodes
# ------------------------------------------------------------------------------------------------
class PairLinearFn(torch.autograd.Function):
    """[y1 | y2 | 0] = x [W1; W2]^T + [b1; b2] in fp32: two heads behind one activation as ONE product (the RPN's
    cls_logits / bbox_pred 1 x 1 convolutions, the box predictor's cls_score / bbox_pred).  The concatenated operand,
    its rows padded to a multiple of 8, lives in the derived-weight cache; the parameters keep their own keys."""

    @staticmethod
    def forward(ctx, x, w1, b1, w2, b2, dtype, sink, lp):
        x2 = x.contiguous().view(-1, x.shape[-1])
        assert x2.dtype == dtype
        n1, n2, k = w1.shape[0], w2.shape[0], x2.shape[1]
        npad = -(-(n1 + n2) // 8) * 8

        def pack(w1, w2, b1, b2):
            w = torch.zeros(npad, k, dtype=torch.float32, device=x2.device)
            w[:n1], w[n1:n1 + n2] = w1.view(n1, k), w2.view(n2, k)
            b = torch.zeros(npad, dtype=torch.float32, device=x2.device)
            b[:n1], b[n1:n1 + n2] = b1, b2
            return (w if dtype == torch.float32 else ops.cast(w, dtype)), b
        wcat, bcat = lp.derived((w1, w2, b1, b2), "pair", dtype, pack)
        ctx.save_for_backward(x2, w1, b1, w2, b2)
        ctx.cfg = (wcat, dtype, sink, x.shape, n1, n2)
        return ops.linear_fwd(x2, wcat, bcat, out_dtype=torch.float32)

    @staticmethod
    def backward(ctx, dy):
        x2, w1, b1, w2, b2 = ctx.saved_tensors
        wcat, dtype, sink, shp, n1, n2 = ctx.cfg
        dy2 = dy.contiguous()
        if dtype != torch.float32:
            _, dy2 = ops.add_cast(dy2, None, want_f32=False, lp_dtype=dtype)
        dx = ops.linear_bwd_data(dy2, wcat).view(shp) if ctx.needs_input_grad[0] else None
        db = torch.empty(dy2.shape[1], dtype=torch.float32, device=dy2.device)
        dw = ops.linear_bwd_weight(dy2, x2, bias_out=db)
        (t1, tb1, t2, tb2), acc, rets = sink.plan([w1, b1, w2, b2])
        for t, v in ((t1, dw[:n1]), (tb1, db[:n1]), (t2, dw[n1:n1 + n2]), (tb2, db[n1:n1 + n2])):
            if t is not None:
                _write_grad(t.view(v.shape), v, acc)
        return dx, rets[0], rets[1], rets[2], rets[3], None, None, None


class ReluFn(torch.autograd.Function):
    """ReLU between two of the heads' products on the library's elementwise kernel (ssl4gie_eltwise op 1,
    out = a > 0 ? b : 0, with a = b = x forward and b = dy backward)"""

    @staticmethod
    def forward(ctx, x):
        x = x.contiguous()
        ctx.save_for_backward(x)
        return ops.relu_bwd(x, x)

    @staticmethod
    def backward(ctx, dy):
        (x,) = ctx.saved_tensors
        return ops.relu_bwd(x, dy.contiguous())


class RoIAlignFn(torch.autograd.Function):
    """MultiScaleRoIAlign(["0", "1", "2", "3"], 7, 2) on the four channels-last fp32 maps -> [K, C * 49] in the GEMM's
    operand type.  The backward adds into zeroed maps with float atomics: not bitwise reproducible."""

    @staticmethod
    def forward(ctx, rois, roi_batch, scales, out_dtype, m0, m1, m2, m3):
        maps = [m.detach() for m in (m0, m1, m2, m3)]
        ctx.save_for_backward(rois, roi_batch)
        ctx.cfg = (scales, [(m.shape, m.stride()) for m in maps])
        return ops.roi_align_fwd(maps, scales, rois, roi_batch, out_dtype)

    @staticmethod
    def backward(ctx, dy):
        rois, roi_batch = ctx.saved_tensors
        scales, geo = ctx.cfg
        dmaps = [torch.zeros(shape[0], shape[2], shape[3], shape[1], dtype=torch.float32,
                             device=dy.device).permute(0, 3, 1, 2) for shape, _ in geo]
        ops.roi_align_bwd(dmaps, scales, rois, roi_batch, dy.contiguous())
        return (None, None, None, None, *dmaps)


# ------------------------------------------------------------------------------------------------
# parameter containers (torchvision's module names, hence its state_dict keys)
# ------------------------------------------------------------------------------------------------
class RPNHead(nn.Module):
    def __init__(self, in_channels, num_anchors):
        super().__init__()
        self.conv = nn.Conv2d(in_channels, in_channels, 3, 1, 1)
        self.cls_logits = nn.Conv2d(in_channels, num_anchors, 1)
        self.bbox_pred = nn.Conv2d(in_channels, num_anchors * 4, 1)
        for layer in self.children():
            nn.init.normal_(layer.weight, std=0.01)
            nn.init.constant_(layer.bias, 0)


class _RPN(nn.Module):
    def __init__(self, in_channels, num_anchors):
        super().__init__()
        self.head = RPNHead(in_channels, num_anchors)


class TwoMLPHead(nn.Module):
    def __init__(self, in_channels, representation_size):
        super().__init__()
        self.fc6 = nn.Linear(in_channels, representation_size)
        self.fc7 = nn.Linear(representation_size, representation_size)


class FastRCNNPredictor(nn.Module):
    def __init__(self, in_channels, num_classes):
        super().__init__()
        self.cls_score = nn.Linear(in_channels, num_classes)
        self.bbox_pred = nn.Linear(in_channels, num_classes * 4)


class _RoIHeads(nn.Module):
    def __init__(self, in_channels, representation_size, num_classes):
        super().__init__()
        self.box_head = TwoMLPHead(in_channels * POOL * POOL, representation_size)
        self.box_predictor = FastRCNNPredictor(representation_size, num_classes)


class _Transform:
    """GeneralizedRCNNTransform reduced to what the reference's loaders need: normalise, and accept only images that
    are already fixed_size (they pad to exactly that); no resize, so postprocess rescaling is the identity."""

    def __init__(self, image_mean, image_std):
        self.image_mean, self.image_std = list(image_mean), list(image_std)
        self.fixed_size = None
        self._dev = {}   # (device, mean, std) -> the two [1, 3, 1, 1] tensors: uploaded once, not per forward

    def batch(self, images):
        if isinstance(images, torch.Tensor):
            images = list(images)
        if not images:
            raise ValueError("FasterRCNN needs at least one image")
        x0 = images[0]
        if self.fixed_size is None:
            raise NotImplementedError("FasterRCNN: set model.transform.fixed_size = (F, F); the transform does not resize")
        Fh, Fw = self.fixed_size
        for im in images:
            if im.dim() != 3 or im.shape[0] != 3:
                raise ValueError(f"images must be [3, H, W], got {tuple(im.shape)}")
            if Fh != Fw or tuple(im.shape[1:]) != (Fh, Fw):
                raise NotImplementedError(f"FasterRCNN accepts only images already {Fh} x {Fw} (square); got "
                                          f"{tuple(im.shape[1:])}: resizing / batching images of differing sizes is not "
                                          "built")
        n = x0.numel() * x0.element_size()
        if all(im.is_contiguous() and im.dtype == x0.dtype and im.device == x0.device and
               im.data_ptr() == x0.data_ptr() + i * n for i, im in enumerate(images)) and \
                x0.untyped_storage().nbytes() - (x0.data_ptr() - x0.untyped_storage().data_ptr()) >= n * len(images):
            return torch.as_strided(x0, (len(images), 3, Fh, Fw), (3 * Fh * Fw, Fh * Fw, Fw, 1))  # views of one batch
        return torch.stack(images)

    def __call__(self, images):
        x = self.batch(images).float()
        key = (str(x.device), tuple(self.image_mean), tuple(self.image_std))
        if key not in self._dev:
            self._dev[key] = tuple(torch.as_tensor(v, dtype=torch.float32, device=x.device)[None, :, None, None]
                                   for v in (self.image_mean, self.image_std))
        mean, std = self._dev[key]
        return (x - mean) / std


# ------------------------------------------------------------------------------------------------
# training-only logic (torch ops on the device, no host wait)
# ------------------------------------------------------------------------------------------------
def match(mqm, high, low, allow_low_quality):
    """torchvision's Matcher on a [G, N] quality matrix: int64 [N], -1 below `low`, -2 between the thresholds"""
    vals, matches = mqm.max(dim=0)
    all_matches = matches.clone()
    matches = torch.where(vals < low, torch.full_like(matches, -1), matches)
    matches = torch.where((vals >= low) & (vals < high), torch.full_like(matches, -2), matches)
    if allow_low_quality:
        best = mqm.max(dim=1).values
        lowq = (mqm == best[:, None]).any(dim=0)
        matches = torch.where(lowq, all_matches, matches)
    return matches


def balanced_sample(labels, batch_size, positive_fraction, keys=None):
    """BalancedPositiveNegativeSampler on one image's labels (>= 1 positive, 0 negative, -1 ignored): two bool masks.
    A random subset of each kind by random keys and ranks; torchvision's random sequence is not reproduced.  keys: fp32
    [n] in [0, 1) instead of the random draw (a test fixes the sample with them)."""
    pos, neg = labels >= 1, labels == 0
    npos = pos.sum().clamp(max=int(batch_size * positive_fraction))
    nneg = neg.sum().clamp(max=batch_size - npos)
    r = torch.rand(labels.shape[0], device=labels.device) if keys is None else keys
    n = labels.shape[0]
    ar = torch.arange(n, device=labels.device)

    def pick(m, cnt):
        order = torch.where(m, r, torch.full_like(r, 2.0)).argsort()
        rank = torch.empty_like(ar).scatter_(0, order, ar)
        return m & (rank < cnt)

    return pick(pos, npos), pick(neg, nneg)


def _first_k(s, k):
    """the k largest of every row, best first, equal values in index order (torch.topk leaves the tie order open)"""
    val, ind = s.sort(dim=1, descending=True, stable=True)
    return val[:, :k], ind[:, :k]


class FasterRCNN(EngineModule):
    """torchvision.models.detection.faster_rcnn.FasterRCNN(backbone, num_classes, ...) for a backbone that yields the
    {"0", "1", "2", "3", "pool"} pyramid (Models.models._ViTBackbone(det=True))."""

    def __init__(self, backbone, num_classes=None, min_size=800, max_size=1333, image_mean=None, image_std=None,
                 rpn_anchor_generator=None, rpn_head=None, rpn_pre_nms_top_n_train=2000, rpn_pre_nms_top_n_test=1000,
                 rpn_post_nms_top_n_train=2000, rpn_post_nms_top_n_test=1000, rpn_nms_thresh=0.7,
                 rpn_fg_iou_thresh=0.7, rpn_bg_iou_thresh=0.3, rpn_batch_size_per_image=256,
                 rpn_positive_fraction=0.5, rpn_score_thresh=0.0, box_roi_pool=None, box_head=None, box_predictor=None,
                 box_score_thresh=0.05, box_nms_thresh=0.5, box_detections_per_img=100, box_fg_iou_thresh=0.5,
                 box_bg_iou_thresh=0.5, box_batch_size_per_image=512, box_positive_fraction=0.25,
                 bbox_reg_weights=None):
        super().__init__()
        if any(a is not None for a in (rpn_anchor_generator, rpn_head, box_roi_pool, box_head, box_predictor)):
            raise NotImplementedError("FasterRCNN: custom anchor generators / heads / poolers are not built")
        if num_classes is None or num_classes < 2:
            raise ValueError("num_classes (background included) must be given")
        if not hasattr(backbone, "out_channels"):
            raise ValueError("backbone should contain an attribute out_channels")
        self.backbone = backbone
        if isinstance(backbone, EngineModule):
            self.adopt(backbone)   # one arena, one gradient sink, one precision for the whole detector
        C = backbone.out_channels
        self.num_classes = num_classes
        self.rpn = _RPN(C, len(ANCHOR_RATIOS))
        self.roi_heads = _RoIHeads(C, 1024, num_classes)
        self.transform = _Transform(image_mean if image_mean is not None else [0.485, 0.456, 0.406],
                                    image_std if image_std is not None else [0.229, 0.224, 0.225])
        self.cfg = dict(pre=(rpn_pre_nms_top_n_train, rpn_pre_nms_top_n_test),
                        post=(rpn_post_nms_top_n_train, rpn_post_nms_top_n_test), rpn_nms=rpn_nms_thresh,
                        rpn_match=(rpn_fg_iou_thresh, rpn_bg_iou_thresh),
                        rpn_sample=(rpn_batch_size_per_image, rpn_positive_fraction), rpn_score=rpn_score_thresh,
                        rpn_min_size=1e-3, box_score=box_score_thresh, box_nms=box_nms_thresh,
                        box_dets=box_detections_per_img, box_match=(box_fg_iou_thresh, box_bg_iou_thresh),
                        box_sample=(box_batch_size_per_image, box_positive_fraction), box_min_size=1e-2,
                        box_weights=tuple(bbox_reg_weights) if bbox_reg_weights is not None else (10.0, 10.0, 5.0, 5.0))
        self._base = base_anchors()
        self._static = {}   # per device: segment offsets and the anchor table, uploaded / built once

    # ------------------------------------------------------------------ kernels or their torch formulations
    def _nms(self, boxes, seg_off, thr, valid, max_seg):
        if _fused(boxes):
            return ops.nms_segments(boxes, seg_off, thr, valid, max_seg)
        return nms_segments_torch(boxes, seg_off, thr, valid, max_seg)

    def _rpn_decode(self, heads, grids, k_off, topk_idx, F):
        fn = ops.rpn_decode if _fused(topk_idx) else rpn_decode_torch
        return fn(heads, grids, k_off, self._base, topk_idx, F, self.cfg["rpn_min_size"], self.cfg["rpn_score"])

    def _roi_decode(self, props, logits, deltas, F):
        fn = ops.roi_decode if _fused(props) else roi_decode_torch
        return fn(props, logits, deltas, self.cfg["box_weights"], F, F, self.cfg["box_min_size"], self.cfg["box_score"])

    def _roi_align(self, maps, scales, rois, roi_batch):
        if _fused(rois):
            return RoIAlignFn.apply(rois, roi_batch, scales, self.dtype_, *maps)
        return roi_align_torch(maps, scales, rois, roi_batch, self.dtype_)

    def _seg_off(self, key, offsets, device):
        k = (key, str(device))
        if k not in self._static:
            self._static[k] = torch.tensor(offsets, dtype=torch.int32, device=device)
        return self._static[k]

    def _anchors(self, grids, F, device):
        """all anchors of the pyramid, fp32 [sum g * g * A, 4] on the device (training only: the matcher needs them)"""
        k = (("anchors", tuple(grids), F), str(device))
        if k not in self._static:
            self._static[k] = torch.cat(grid_anchors(self._base, grids, F, device), 0)
        return self._static[k]

    # overridable: a test fixes the sample through these
    def sample_rpn(self, labels):
        return balanced_sample(labels, *self.cfg["rpn_sample"])

    def sample_roi(self, labels):
        return balanced_sample(labels, *self.cfg["box_sample"])

    # ------------------------------------------------------------------ RPN
    def rpn_head(self, features):
        """Conv3x3 + ReLU over the five levels, then the two 1 x 1 heads as one product: a list of fp32
        [B * g * g, 16] (columns [0, 3) objectness logits, [3, 15) the deltas of the three anchors) and the grid sides"""
        from ..dpt_engine import Conv3x3Fn
        h, dt, sink, lp = self.rpn.head, self.dtype_, self.sink(), self.lp_cache
        outs, grids = [], []
        for m in features.values():
            x = m.permute(0, 2, 3, 1).contiguous().to(dt)
            t = ReluFn.apply(Conv3x3Fn.apply(x, h.conv.weight, h.conv.bias, 1, False, sink, lp))
            outs.append(PairLinearFn.apply(t.reshape(-1, t.shape[-1]), h.cls_logits.weight, h.cls_logits.bias,
                                           h.bbox_pred.weight, h.bbox_pred.bias, dt, sink, lp))
            grids.append(m.shape[2])
        return outs, grids

    @torch.no_grad()
    def rpn_candidates(self, heads, grids, B):
        """the best `pre_nms_top_n` candidates per (image, level) by objectness logit: indices int64 [B, Ktot] inside
        their level, best first, and the levels' ranges k_off (Python ints).  A stable sort, not torch.topk (whose tie
        order is unspecified): equal logits keep the lower index first, which is the order the NMS is specified for."""
        A = self._base.shape[1]
        pre = self.cfg["pre"][0 if self.training else 1]
        idx, k_off = [], [0]
        for h, g in zip(heads, grids):
            k = min(pre, g * g * A)
            order = h.detach()[:, :A].reshape(B, g * g * A).sort(dim=1, descending=True, stable=True).indices
            idx.append(order[:, :k])
            k_off.append(k_off[-1] + k)
        return torch.cat(idx, 1), k_off

    def rpn_segments(self, B, k_off, device):
        """one NMS segment per (image, level): int32 [B * L + 1] on the device, and the longest segment"""
        ktot = k_off[-1]
        seg = self._seg_off(("rpn", B, tuple(k_off)), [b * ktot + k for b in range(B) for k in k_off[:-1]] + [B * ktot],
                            device)
        return seg, max(b - a for a, b in zip(k_off, k_off[1:]))

    @torch.no_grad()
    def rpn_proposals(self, heads, grids, B, F):
        """RegionProposalNetwork.filter_proposals with static shapes: proposals fp32 [B, P, 4] (zero boxes beyond the
        kept ones), flags bool [B, P], scores fp32 [B, P]; P = post_nms_top_n (or every candidate, if fewer)"""
        post = self.cfg["post"][0 if self.training else 1]
        topk_idx, k_off = self.rpn_candidates(heads, grids, B)
        ktot = k_off[-1]
        boxes, scores, valid = self._rpn_decode([h.detach() for h in heads], grids, k_off, topk_idx, F)
        seg, max_seg = self.rpn_segments(B, k_off, boxes.device)
        keep_rank, _ = self._nms(boxes.view(-1, 4), seg, self.cfg["rpn_nms"], valid.view(-1), max_seg)
        s = torch.where(keep_rank.view(B, ktot) >= 0, scores, torch.full_like(scores, -1.0))
        val, ind = _first_k(s, min(post, ktot))
        ok = val >= 0
        props = boxes.gather(1, ind[:, :, None].expand(-1, -1, 4)) * ok[:, :, None]
        return props, ok, val

    def rpn_targets(self, heads, grids, targets, F):
        """RegionProposalNetwork.assign_targets_to_anchors and the sample: logits [B, N], deltas [B, N, 4] of all anchors
        in torchvision's order, labels fp32 [B, N] (1 / 0 / -1), regression targets [B, N, 4], and the masks of the
        sampled positives and of everything sampled"""
        A = self._base.shape[1]
        B = len(targets)
        dev = heads[0].device
        anchors = self._anchors(grids, F, dev)
        logits = torch.cat([h[:, :A].reshape(B, -1) for h in heads], 1)
        deltas = torch.cat([h[:, A:5 * A].reshape(B, -1, 4) for h in heads], 1)
        hi, lo = self.cfg["rpn_match"]
        lab, reg, pos, sel = [], [], [], []
        for t in targets:
            gt = t["boxes"]
            if gt.shape[0] == 0:
                labels = torch.zeros(anchors.shape[0], device=dev)
                mgt = torch.zeros_like(anchors)
            else:
                m = match(box_iou(gt, anchors), hi, lo, True)
                mgt = gt[m.clamp(min=0)]
                labels = (m >= 0).float()
                labels = torch.where(m == -1, torch.zeros_like(labels), labels)
                labels = torch.where(m == -2, torch.full_like(labels, -1.0), labels)
            p, n = self.sample_rpn(labels)
            lab.append(labels)
            reg.append(encode_boxes(mgt, anchors, (1.0, 1.0, 1.0, 1.0)))
            pos.append(p)
            sel.append(p | n)
        return logits, deltas, torch.stack(lab), torch.stack(reg), torch.stack(pos), torch.stack(sel)

    # ------------------------------------------------------------------ RoI heads
    def box_head(self, features, rois, roi_batch, F):
        """RoIAlign -> fc6 -> ReLU -> fc7 -> ReLU -> [cls_score | bbox_pred] as one product: fp32 [K, >= 5 C]"""
        maps = [features[k] for k in ("0", "1", "2", "3")]
        scales = [2.0 ** round(math.log2(m.shape[2] / F)) for m in maps]
        x = self._roi_align(maps, scales, rois, roi_batch)
        bh, bp = self.roi_heads.box_head, self.roi_heads.box_predictor
        x = ReluFn.apply(self._lin(x, bh.fc6))
        x = ReluFn.apply(self._lin(x, bh.fc7))
        return PairLinearFn.apply(x, bp.cls_score.weight, bp.cls_score.bias, bp.bbox_pred.weight, bp.bbox_pred.bias,
                                  self.dtype_, self.sink(), self.lp_cache)

    def _lin(self, x, lin):
        return LinearFn.apply(x, lin.weight, lin.bias, self.dtype_, self.dtype_, self.sink(), self.lp_cache)

    @torch.no_grad()
    def select_training_samples(self, props, ok, targets):
        """RoIHeads.select_training_samples with static shapes: the ground truths are appended to the (detached)
        proposals, matched (0.5, 0.5), sampled, and the sampled RoIs gathered to the front: rois [B, S, 4], labels int64
        [B, S], regression targets [B, S, 4], flags bool [B, S]; S = batch_size_per_image (or every RoI, if fewer)"""
        hi, lo = self.cfg["box_match"]
        R, L, T, V = [], [], [], []
        for b, t in enumerate(targets):
            gt, gl = t["boxes"].to(props.dtype), t["labels"]
            rois = torch.cat([props[b], gt], 0)
            live = torch.cat([ok[b], torch.ones(gt.shape[0], dtype=torch.bool, device=ok.device)])
            if gt.shape[0] == 0:
                labels = torch.zeros(rois.shape[0], dtype=torch.int64, device=rois.device)
                mgt = torch.zeros_like(rois)
            else:
                m = match(box_iou(gt, rois), hi, lo, False)
                labels = gl[m.clamp(min=0)].to(torch.int64)
                labels = torch.where(m == -1, torch.zeros_like(labels), labels)
                labels = torch.where(m == -2, torch.full_like(labels, -1), labels)
                mgt = gt[m.clamp(min=0)]
            labels = torch.where(live, labels, torch.full_like(labels, -1))
            p, n = self.sample_roi(labels)
            s = p | n
            S = min(self.cfg["box_sample"][0], rois.shape[0])
            idx = s.to(torch.uint8).argsort(descending=True, stable=True)[:S]
            sv = s[idx]
            rr = rois[idx] * sv[:, None]
            tt = encode_boxes(mgt[idx], rois[idx], self.cfg["box_weights"])
            R.append(rr)
            L.append(torch.where(sv, labels[idx], torch.zeros_like(labels[idx])))
            T.append(torch.where((sv & (labels[idx] > 0))[:, None], tt, torch.zeros_like(tt)))
            V.append(sv)
        return torch.stack(R), torch.stack(L), torch.stack(T), torch.stack(V)

    @torch.no_grad()
    def box_candidates(self, out, props, ok, F):
        """the detection stage up to the NMS: per-class boxes decoded and flagged, then one segment per (image, class)
        sorted by descending score (stable: equal scores keep the lower index first).  Returns boxes fp32
        [B, C - 1, P, 4], scores fp32 [B, C - 1, P] (-1 for a box that is not valid), flags uint8 [B, C - 1, P]"""
        B, P = ok.shape
        C = self.num_classes
        boxes, scores, valid = self._roi_decode(props.reshape(-1, 4).contiguous(), out[:, :C], out[:, C:5 * C], F)
        valid = valid.view(B, P, C - 1).bool() & ok[:, :, None]
        s = torch.where(valid, scores.view(B, P, C - 1), torch.full_like(scores.view(B, P, C - 1), -1.0))
        s, order = s.permute(0, 2, 1).sort(dim=-1, descending=True, stable=True)
        bs = boxes.view(B, P, C - 1, 4).permute(0, 2, 1, 3).gather(2, order[..., None].expand(-1, -1, -1, 4)).contiguous()
        return bs, s.contiguous(), (s >= 0).to(torch.uint8).contiguous()

    @torch.no_grad()
    def postprocess(self, out, props, ok, F):
        """RoIHeads.postprocess_detections with static shapes: boxes [B, D, 4], scores [B, D], labels int64 [B, D] and
        the number of detections per image, int64 [B] (on the device)"""
        B, P = ok.shape
        C = self.num_classes
        bs, s, vs = self.box_candidates(out, props, ok, F)
        n = B * (C - 1)
        seg = self._seg_off(("box", n, P), [i * P for i in range(n + 1)], out.device)
        keep_rank, _ = self._nms(bs.view(-1, 4), seg, self.cfg["box_nms"], vs.view(-1), P)
        s = torch.where(keep_rank.view(B, C - 1, P) >= 0, s, torch.full_like(s, -1.0)).reshape(B, -1)
        val, ind = _first_k(s, min(self.cfg["box_dets"], s.shape[1]))
        labels = torch.div(ind, P, rounding_mode="floor") + 1
        db = bs.view(B, -1, 4).gather(1, ind[:, :, None].expand(-1, -1, 4))
        return db, val, labels, (val >= 0).sum(1)

    # ------------------------------------------------------------------ forward
    def forward(self, images, targets=None):
        if self.training and targets is None:
            raise ValueError("In training mode, targets should be passed")
        self._prepare()
        x = self.transform(images)
        B, F = x.shape[0], x.shape[-1]
        features = self.backbone(x)
        if isinstance(features, torch.Tensor):
            features = OrderedDict([("0", features)])
        heads, grids = self.rpn_head(features)
        props, ok, _ = self.rpn_proposals(heads, grids, B, F)
        if self.training:
            rois, labels, reg, sv = self.select_training_samples(props, ok, targets)
            S = rois.shape[1]
            roi_batch = torch.arange(B, dtype=torch.int32, device=x.device).repeat_interleave(S)
            out = self.box_head(features, rois.reshape(-1, 4).contiguous(), roi_batch, F)
            C = self.num_classes
            lc, lb = fastrcnn_loss(out[:, :C], out[:, C:5 * C], labels.view(-1), reg.view(-1, 4), sv.view(-1))
            lo, lr = rpn_loss(*self.rpn_targets(heads, grids, targets, F))
            return {"loss_classifier": lc, "loss_box_reg": lb, "loss_objectness": lo, "loss_rpn_box_reg": lr}
        P = props.shape[1]
        roi_batch = torch.arange(B, dtype=torch.int32, device=x.device).repeat_interleave(P)
        out = self.box_head(features, props.reshape(-1, 4).contiguous(), roi_batch, F)
        db, ds, dl, cnt = self.postprocess(out, props, ok, F)
        cnt = cnt.tolist()   # the one read-back: the result list is split per image
        return [{"boxes": db[b, :c], "labels": dl[b, :c], "scores": ds[b, :c]} for b, c in enumerate(cnt)]


def rpn_loss(logits, deltas, labels, reg, pos, sel):
    """RegionProposalNetwork.compute_loss on masks: BCE-with-logits over the sampled anchors (mean), smooth-L1 with
    beta = 1 / 9 over the positive ones, summed and divided by the number sampled"""
    n = sel.sum().clamp(min=1).float()
    reg = torch.where(pos[..., None], reg, torch.zeros_like(reg))
    box = F_.smooth_l1_loss(deltas, reg, beta=1 / 9, reduction="none")
    box = torch.where(pos[..., None], box, torch.zeros_like(box)).sum() / n
    obj = F_.binary_cross_entropy_with_logits(logits, labels.clamp(min=0), reduction="none")
    obj = torch.where(sel, obj, torch.zeros_like(obj)).sum() / n
    return obj, box


def fastrcnn_loss(class_logits, box_regression, labels, reg, sel):
    """roi_heads.fastrcnn_loss on masks: cross-entropy over the sampled RoIs (mean), class-specific smooth-L1 with
    beta = 1 / 9 over the positive ones, summed and divided by the number sampled"""
    n = sel.sum().clamp(min=1).float()
    ce = F_.cross_entropy(class_logits, labels, reduction="none")
    ce = torch.where(sel, ce, torch.zeros_like(ce)).sum() / n
    K, C4 = box_regression.shape
    pos = sel & (labels > 0)
    pred = box_regression.reshape(K, C4 // 4, 4).gather(1, labels.clamp(min=0)[:, None, None].expand(-1, 1, 4))[:, 0]
    box = F_.smooth_l1_loss(pred, reg, beta=1 / 9, reduction="none")
    box = torch.where(pos[:, None], box, torch.zeros_like(box)).sum() / n
    return ce, box
