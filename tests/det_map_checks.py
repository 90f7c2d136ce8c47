"""fp64 restatement of the detection metric (ssl4gie_amd.metrics.MeanAveragePrecision, csrc/det_map_ops.hip) in
pycocotools' loop order — COCOeval.evaluateImg, .accumulate and .summarize as torchmetrics 1.1.2's defaults drive them —
with numpy and no GPU, plus the case generators of the two test files and `margins`.

A case is a list of images; an image is a dict of numpy arrays: boxes fp32 [n, 4] (xyxy), scores fp32 [n], labels int64
[n] (the detections), gt_boxes fp32 [m, 4], gt_labels int64 [m].

`margins(case)` counts the decisions that an fp rounding could turn: an IoU of a same-class pair closer than 1e-9 to a
threshold, an area closer than 1e-3 px^2 to 32^2 or 96^2.  Every random case asserts 0 ("invalid case")."""
import numpy as np
import torch

IOU_THRS = torch.linspace(0.5, 0.95, 10).tolist()
REC_THRS = torch.linspace(0.0, 1.0, 101).tolist()
AREA_RNG = ((0.0, 1e10), (0.0, 32.0 ** 2), (32.0 ** 2, 96.0 ** 2), (96.0 ** 2, 1e10))
MAX_DETS = (1, 10, 100)
NAMES = ("map", "map_50", "map_75", "map_small", "map_medium", "map_large", "mar_1", "mar_10", "mar_100", "mar_small",
         "mar_medium", "mar_large")
T, R, A, M = len(IOU_THRS), len(REC_THRS), len(AREA_RNG), len(MAX_DETS)


def xywh(boxes):
    """torchvision's box_convert(xyxy -> xywh) on fp32, then Python floats"""
    b = np.asarray(boxes, dtype=np.float32).reshape(-1, 4)
    w = (b[:, 2] - b[:, 0]).astype(np.float32)
    h = (b[:, 3] - b[:, 1]).astype(np.float32)
    return np.stack([b[:, 0].astype(np.float64), b[:, 1].astype(np.float64), w.astype(np.float64),
                     h.astype(np.float64)], 1)


def iou_matrix(d, g):
    """maskUtils.iou on xywh boxes without crowd, [D, G] fp64"""
    out = np.zeros((len(d), len(g)))
    for i in range(len(d)):
        w = np.minimum(d[i, 0] + d[i, 2], g[:, 0] + g[:, 2]) - np.maximum(d[i, 0], g[:, 0])
        h = np.minimum(d[i, 1] + d[i, 3], g[:, 1] + g[:, 3]) - np.maximum(d[i, 1], g[:, 1])
        ok = (w > 0) & (h > 0)
        inter = w * h
        union = d[i, 2] * d[i, 3] + g[:, 2] * g[:, 3] - inter
        out[i, ok] = inter[ok] / union[ok]
    return out


def evaluate_img(img, c, a):
    """COCOeval.evaluateImg for class c and area range a with maxDet = 100; None without detection and ground truth.
    dt_idx: the image's detections of c, best first (their index in the image); dtm / dt_ig bool [T, D]."""
    lo, hi = AREA_RNG[a]
    di = np.nonzero(img["labels"] == c)[0]
    gi = np.nonzero(img["gt_labels"] == c)[0]
    if len(di) == 0 and len(gi) == 0:
        return None
    di = di[np.argsort(-img["scores"][di], kind="mergesort")][:MAX_DETS[-1]]
    d, g = xywh(img["boxes"][di]), xywh(img["gt_boxes"][gi])
    g_area = g[:, 2] * g[:, 3]
    g_ig = np.array([bool(ar < lo or ar > hi) for ar in g_area], dtype=bool)
    gorder = np.argsort(g_ig.astype(np.uint8), kind="mergesort")
    g, g_ig = g[gorder], g_ig[gorder]
    ious = iou_matrix(d, g)
    D, G = len(d), len(g)
    gtm = np.zeros((T, G), dtype=bool)
    dtm = np.zeros((T, D), dtype=bool)
    dt_ig = np.zeros((T, D), dtype=bool)
    cand = [np.nonzero(ious[k] >= 0.5)[0] for k in range(D)]   # below every threshold: `continue` at once in the walk
    for tind, t in enumerate(IOU_THRS):
        for dind in range(D):
            iou = min([t, 1 - 1e-10])
            m = -1
            for gind in cand[dind]:
                if gtm[tind, gind]:
                    continue
                if m > -1 and not g_ig[m] and g_ig[gind]:
                    break
                if ious[dind, gind] < iou:
                    continue
                iou = ious[dind, gind]
                m = gind
            if m == -1:
                continue
            dt_ig[tind, dind] = g_ig[m]
            dtm[tind, dind] = True
            gtm[tind, m] = True
    d_area = d[:, 2] * d[:, 3]
    out = np.array([bool(ar < lo or ar > hi) for ar in d_area], dtype=bool).reshape(1, D)
    dt_ig = np.logical_or(dt_ig, np.logical_and(~dtm, np.repeat(out, T, 0)))
    return {"dt_idx": di, "scores": img["scores"][di], "dtm": dtm, "dt_ig": dt_ig, "g_ig": g_ig, "ious": ious}


def classes_of(case):
    s = set()
    for img in case:
        s.update(int(x) for x in img["labels"])
        s.update(int(x) for x in img["gt_labels"])
    return sorted(s)


def accumulate(case):
    """precision [T, R, K, A, M], recall [T, K, A, M], classes"""
    classes = classes_of(case)
    K = len(classes)
    precision = -np.ones((T, R, K, A, M))
    recall = -np.ones((T, K, A, M))
    for k, c in enumerate(classes):
        for a in range(A):
            E = [evaluate_img(img, c, a) for img in case]
            E = [e for e in E if e is not None]
            if not E:
                continue
            for mi, max_det in enumerate(MAX_DETS):
                scores = np.concatenate([e["scores"][:max_det] for e in E])
                inds = np.argsort(-scores, kind="mergesort")
                dtm = np.concatenate([e["dtm"][:, :max_det] for e in E], axis=1)[:, inds]
                dt_ig = np.concatenate([e["dt_ig"][:, :max_det] for e in E], axis=1)[:, inds]
                g_ig = np.concatenate([e["g_ig"] for e in E])
                npig = np.count_nonzero(~g_ig)
                if npig == 0:
                    continue
                tps = np.logical_and(dtm, ~dt_ig)
                fps = np.logical_and(~dtm, ~dt_ig)
                tp_sum = np.cumsum(tps, axis=1).astype(dtype=float)
                fp_sum = np.cumsum(fps, axis=1).astype(dtype=float)
                for t, (tp, fp) in enumerate(zip(tp_sum, fp_sum)):
                    nd = len(tp)
                    rc = tp / npig
                    pr = tp / (fp + tp + np.spacing(1))
                    q = np.zeros((R,))
                    recall[t, k, a, mi] = rc[-1] if nd else 0
                    pr = pr.tolist()
                    for i in range(nd - 1, 0, -1):
                        if pr[i] > pr[i - 1]:
                            pr[i - 1] = pr[i]
                    inds_r = np.searchsorted(rc, REC_THRS, side="left")
                    for ri, pi in enumerate(inds_r):
                        if pi < nd:
                            q[ri] = pr[pi]
                    precision[t, :, k, a, mi] = q
    return precision, recall, classes


def _mean(s):
    s = s[s > -1]
    return float(np.mean(s)) if s.size else -1.0


def summarize(precision, recall):
    out = {
        "map": _mean(precision[:, :, :, 0, 2]),
        "map_50": _mean(precision[0, :, :, 0, 2]),
        "map_75": _mean(precision[5, :, :, 0, 2]),
        "map_small": _mean(precision[:, :, :, 1, 2]),
        "map_medium": _mean(precision[:, :, :, 2, 2]),
        "map_large": _mean(precision[:, :, :, 3, 2]),
        "mar_1": _mean(recall[:, :, 0, 0]),
        "mar_10": _mean(recall[:, :, 0, 1]),
        "mar_100": _mean(recall[:, :, 0, 2]),
        "mar_small": _mean(recall[:, :, 1, 2]),
        "mar_medium": _mean(recall[:, :, 2, 2]),
        "mar_large": _mean(recall[:, :, 3, 2]),
    }
    return out


def restate(case):
    """the twelve fp64 summaries and the classes"""
    precision, recall, classes = accumulate(case)
    return summarize(precision, recall), classes


def match_all(case):
    """What the match stage gives, per detection in `update` order: rank int64 [N] (stable rank among the same-label
    detections of the image), matched / ignored int64 [N] (bit = area * 10 + threshold; 0 for rank >= 100), and npig
    int64 [256, 4], present int64 [256]."""
    n = [len(img["scores"]) for img in case]
    start = np.concatenate([[0], np.cumsum(n)]).astype(np.int64)
    rank = np.zeros(start[-1], dtype=np.int64)
    matched = np.zeros(start[-1], dtype=np.int64)
    ignored = np.zeros(start[-1], dtype=np.int64)
    npig = np.zeros((256, 4), dtype=np.int64)
    present = np.zeros(256, dtype=np.int64)
    for i, img in enumerate(case):
        for c in sorted(set(img["labels"].tolist()) | set(img["gt_labels"].tolist())):
            present[c] = 1
            di = np.nonzero(img["labels"] == c)[0]
            order = di[np.argsort(-img["scores"][di], kind="mergesort")]
            rank[start[i] + order] = np.arange(len(order))
            for a in range(A):
                e = evaluate_img(img, c, a)
                npig[c, a] += np.count_nonzero(~e["g_ig"])
                for t in range(T):
                    bit = np.int64(1) << np.int64(a * T + t)
                    matched[start[i] + e["dt_idx"][e["dtm"][t]]] |= bit
                    ignored[start[i] + e["dt_idx"][e["dt_ig"][t]]] |= bit
    return rank, matched, ignored, npig, present


def margins(case):
    n = 0
    thr = np.asarray(IOU_THRS)
    for img in case:
        d, g = xywh(img["boxes"]), xywh(img["gt_boxes"])
        for ar in np.concatenate([d[:, 2] * d[:, 3], g[:, 2] * g[:, 3]]):
            n += int(min(abs(ar - 32.0 ** 2), abs(ar - 96.0 ** 2)) < 1e-3)
        if len(d) and len(g):
            ious = iou_matrix(d, g)
            same = img["labels"][:, None] == img["gt_labels"][None, :]
            n += int(np.count_nonzero((np.abs(ious[:, :, None] - thr[None, None, :]) < 1e-9) & same[:, :, None]))
    return n


# ------------------------------------------------------------------ cases
def image(boxes=(), scores=(), labels=(), gt_boxes=(), gt_labels=()):
    return {"boxes": np.asarray(boxes, dtype=np.float32).reshape(-1, 4),
            "scores": np.asarray(scores, dtype=np.float32).reshape(-1),
            "labels": np.asarray(labels, dtype=np.int64).reshape(-1),
            "gt_boxes": np.asarray(gt_boxes, dtype=np.float32).reshape(-1, 4),
            "gt_labels": np.asarray(gt_labels, dtype=np.int64).reshape(-1)}


def _rand_boxes(rng, n, kind=None, canvas=640.0):
    """n xyxy boxes; kind 0 / 1 / 2 = small / medium / large sides, None = any"""
    kinds = rng.integers(0, 3, n) if kind is None else np.full(n, kind)
    lo = np.array([6.0, 40.0, 110.0])[kinds]
    hi = np.array([28.0, 88.0, 300.0])[kinds]
    w, h = rng.uniform(lo, hi), rng.uniform(lo, hi)
    x, y = rng.uniform(0, canvas - w), rng.uniform(0, canvas - h)
    return np.stack([x, y, x + w, y + h], 1).astype(np.float32)


def random_image(rng, n_det, n_gt, labels=(1, 2, 7), kinds=None, tie_scores=True):
    labels = np.asarray(labels)
    gt_boxes = _rand_boxes(rng, n_gt) if kinds is None else \
        np.concatenate([_rand_boxes(rng, 1, k) for k in kinds] + [_rand_boxes(rng, max(0, n_gt - len(kinds)))])[:n_gt]
    gt_boxes = gt_boxes.reshape(-1, 4)
    gt_labels = labels[rng.integers(0, len(labels), n_gt)]
    boxes = _rand_boxes(rng, n_det)
    det_labels = labels[rng.integers(0, len(labels), n_det)]
    if n_gt:
        # most detections are shifted, rescaled copies of a ground truth, some with the wrong label
        src = rng.integers(0, n_gt, n_det)
        near = rng.random(n_det) < 0.7
        g = gt_boxes[src].astype(np.float64)
        w, h = g[:, 2] - g[:, 0], g[:, 3] - g[:, 1]
        shift = rng.uniform(-0.25, 0.25, (n_det, 2)) * np.stack([w, h], 1) * rng.random((n_det, 1))
        scale = rng.uniform(0.8, 1.25, (n_det, 2))
        cx, cy = (g[:, 0] + g[:, 2]) / 2 + shift[:, 0], (g[:, 1] + g[:, 3]) / 2 + shift[:, 1]
        nb = np.stack([cx - w * scale[:, 0] / 2, cy - h * scale[:, 1] / 2, cx + w * scale[:, 0] / 2,
                       cy + h * scale[:, 1] / 2], 1).astype(np.float32)
        boxes[near] = nb[near]
        keep_label = near & (rng.random(n_det) < 0.85)
        det_labels[keep_label] = gt_labels[src[keep_label]]
    scores = rng.random(n_det)
    if tie_scores:
        scores = np.round(scores * 32) / 32     # ties within and across images: the stable orders decide
    return image(boxes, scores, det_labels, gt_boxes, gt_labels)


RANDOM_DET_COUNTS = (0, 1, 5, 63, 64, 65, 100, 130)


def random_case(seed, n_img=12, labels=(1, 2, 7)):
    """12 images, labels {1, 2, 7}, detection counts from RANDOM_DET_COUNTS (every one used), 0-5 boxes, all three
    area ranges populated"""
    rng = np.random.default_rng(seed)
    counts = list(RANDOM_DET_COUNTS) + [int(x) for x in rng.choice(RANDOM_DET_COUNTS, max(0, n_img - 8))]
    counts = [counts[i] for i in rng.permutation(len(counts))][:n_img]
    case = []
    for i, nd in enumerate(counts):
        n_gt = int(rng.integers(0, 6)) if i else 5
        case.append(random_image(rng, nd, n_gt, labels, kinds=(0, 1, 2) if i == 0 else None))
    return case


def docstring_case():
    return [image([[258.0, 41.0, 606.0, 285.0]], [0.536], [0], [[214.0, 41.0, 562.0, 285.0]], [0])]


def to_updates(case, device="cpu"):
    """(preds, target) lists for MeanAveragePrecision.update"""
    preds = [{"boxes": torch.from_numpy(i["boxes"]).to(device), "scores": torch.from_numpy(i["scores"]).to(device),
              "labels": torch.from_numpy(i["labels"]).to(device)} for i in case]
    target = [{"boxes": torch.from_numpy(i["gt_boxes"]).to(device), "labels": torch.from_numpy(i["gt_labels"]).to(device)}
              for i in case]
    return preds, target


def flat(case, device="cpu"):
    """the end-to-end arrays of ops.det_map_match: det boxes, scores, labels, offsets, gt boxes, labels, offsets"""
    def cat(key, shape, dt):
        return torch.from_numpy(np.concatenate([i[key] for i in case]).astype(dt).reshape(shape)).to(device)

    def off(key):
        return torch.tensor(np.concatenate([[0], np.cumsum([len(i[key]) for i in case])]), dtype=torch.int32).to(device)
    return (cat("boxes", (-1, 4), np.float32), cat("scores", (-1,), np.float32), cat("labels", (-1,), np.int64),
            off("scores"), cat("gt_boxes", (-1, 4), np.float32), cat("gt_labels", (-1,), np.int64), off("gt_labels"))


def shape_case(labels=(1, 2, 7), seed=11):
    """detection counts 0 / 1 / 63 / 64 / 65 / 100 / 101 / 130 / 1024 against ground-truth counts 0 / 1 / 17 / 1024"""
    rng = np.random.default_rng(seed)
    pairs = ((0, 0), (1, 1), (63, 17), (64, 0), (65, 1), (100, 17), (101, 1), (130, 17), (1024, 1), (5, 1024),
             (1024, 1024), (0, 17))
    return [random_image(rng, nd, ng, labels) for nd, ng in pairs]


def exact_case():
    """boxes identical to their ground truth (IoU exactly 1), twice each, and degenerate zero-area boxes on both sides"""
    rng = np.random.default_rng(5)
    g = _rand_boxes(rng, 6)
    flat_boxes = np.array([[10, 10, 10, 40], [50, 60, 90, 60], [7, 7, 7, 7]], dtype=np.float32)
    return [image(np.concatenate([g, g]), np.linspace(0.9, 0.1, 12), [3] * 12, g, [3] * 6),
            image(np.concatenate([flat_boxes, g[:2]]), [0.5, 0.4, 0.3, 0.2, 0.1], [3] * 5,
                  np.concatenate([flat_boxes, g[:1]]), [3] * 4)]


def segment_case(chunk=256, seed=21):
    """class segments of length 0 (class 0: ground truths only), 1, chunk - 1, chunk, chunk + 1, 2 * chunk + 1
    (classes 1 - 5) and a class without ground truth (6: npig == 0), over four images"""
    rng = np.random.default_rng(seed)
    totals = {0: 0, 1: 1, 2: chunk - 1, 3: chunk, 4: chunk + 1, 5: 2 * chunk + 1, 6: 40}
    n_img = 6
    case = []
    left = dict(totals)
    for i in range(n_img):
        boxes, scores, labels, gtb, gtl = [], [], [], [], []
        for c, _ in totals.items():
            n = min(100, left[c])
            left[c] -= n
            g = _rand_boxes(rng, 0 if c == 6 else 2)
            gtb.append(g)
            gtl += [c] * len(g)
            sub = random_image(rng, n, len(g), (c,))
            if len(g) and n:   # detections around this class's boxes
                src = rng.integers(0, len(g), n)
                jit = rng.uniform(-0.2, 0.2, (n, 4)) * np.tile(g[src][:, 2:] - g[src][:, :2], 2)
                near = rng.random(n) < 0.6
                sub["boxes"][near] = (g[src] + jit)[near].astype(np.float32)
            boxes.append(sub["boxes"])
            scores.append(sub["scores"])
            labels += [c] * n
        case.append(image(np.concatenate(boxes), np.concatenate(scores), labels, np.concatenate(gtb), gtl))
    assert all(v == 0 for v in left.values())
    return case


def fused_iou(d, g):
    """bbIou of two xywh boxes as a build with contracted arithmetic computes it: the union as one fused
    multiply-add, fma(-w, h, area + area'), which subtracts the UNROUNDED intersection.  Exact rationals, rounded once."""
    from fractions import Fraction
    w = min(d[0] + d[2], g[0] + g[2]) - max(d[0], g[0])
    h = min(d[1] + d[3], g[1] + g[3]) - max(d[1], g[1])
    if w <= 0 or h <= 0:
        return 0.0
    return (w * h) / float(Fraction(d[2] * d[3] + g[2] * g[3]) - Fraction(w) * Fraction(h))


# (x1, y1 of the detection), found by search: with the detection [x1, y1, 96, H] and the ground truth [GX, 0, GX + 96, H]
# the overlap's sides carry about 50 significant bits, their product is inexact in fp64, and the IoU rounded operation
# by operation is exactly 0.75 — the sixth threshold — while with the fused union it is 0.75 - 2^-53
ROUNDING_H = float.fromhex("0x1.488c160000000p+5")
ROUNDING_GX = float.fromhex("0x1.b6db700000000p+3")
ROUNDING_XY = (("0x1.2ceb080000000p-19", "0x1.34b4800000000p-21"), ("0x1.8c61360000000p-19", "0x1.f348680000000p-21"),
               ("0x1.559bcc0000000p-19", "0x1.85f0540000000p-21"), ("0x1.c019340000000p-19", "0x1.2d443c0000000p-20"))


def rounding_case():
    """Detections whose IoU with their ground truth is exactly the threshold 0.75 when every fp64 operation is rounded
    on its own, and one ulp below it when the union is contracted into a fused multiply-add: the match at threshold
    index 5 tells the two apart.  One pair per image, and all four pairs once more in one image under another label."""
    H, gx = ROUNDING_H, ROUNDING_GX
    gt = [gx, 0.0, gx + 96.0, H]
    dets = [[float.fromhex(x), float.fromhex(y), 96.0, H] for x, y in ROUNDING_XY]
    case = [image([d], [0.9], [2], [gt], [2]) for d in dets]
    case.append(image(dets, [0.9, 0.8, 0.7, 0.6], [4] * 4, [gt], [4]))
    return case
