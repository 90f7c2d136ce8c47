"""GPU: the Faster R-CNN head kernels (csrc/det_head_ops.hip) against the fp64 restatements of det_head_checks.py —
integers and flags held to equality, values to gates computed from the fp32 torch formulation's own distance from fp64
— and ssl4gie_amd.Models.detection.FasterRCNN stage by stage, in training, in eval and over a few optimizer steps."""
import functools
import math

import numpy as np
import pytest
import torch

import det_head_checks as chk
from ssl4gie_amd import ops
from ssl4gie_amd.Models import detection as det

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _t(a, dtype=None):
    return torch.as_tensor(a, dtype=dtype).to(DEV)


# ------------------------------------------------------------------ NMS
@pytest.mark.parametrize("thr,sizes,seed", [(0.7, (1, 63, 0, 64, 65, 257, 2000, 4096), 11), (0.5, (65, 0, 300, 2), 12)])
def test_nms_segments_random(thr, sizes, seed):
    """segment sizes around the 64-box word and block boundaries up to the 4096 cap, an empty segment among them, with
    and without validity flags: keep ranks and counts equal the fp64 greedy sweep"""
    boxes, seg_off, valid = chk.nms_case(sizes, thr, seed)
    for v in (valid, None):
        rank, cnt = chk.nms_ref(boxes, seg_off, thr, v)
        got, gc = ops.nms_segments(_t(boxes), _t(seg_off), thr, None if v is None else _t(v), max_seg=max(sizes))
        assert np.array_equal(got.cpu().numpy(), rank)
        assert np.array_equal(gc.cpu().numpy(), cnt)
    # a bound below the longest segment: only its first max_seg boxes take part; without a bound the offsets are read
    got, _ = ops.nms_segments(_t(boxes), _t(seg_off), thr, _t(valid))
    assert np.array_equal(got.cpu().numpy(), chk.nms_ref(boxes, seg_off, thr, valid)[0])


def test_nms_segments_crafted():
    boxes, seg_off = chk.nms_exact_case()
    # IoU exactly 0.5 and exactly 0.7: intersection, union and quotient are exact in fp32, `>` keeps those boxes
    assert ops.nms_segments(_t(boxes), _t(seg_off), 0.5)[0].tolist() == [0, 1, 0, -1]
    assert ops.nms_segments(_t(boxes), _t(seg_off), 0.7)[0].tolist() == [0, 1, 0, 1]
    # A suppresses B, B would have suppressed C: C is kept
    boxes, seg_off = chk.nms_chain_case()
    rank, cnt = ops.nms_segments(_t(boxes), _t(seg_off), 0.5)
    assert rank.tolist() == [0, -1, 1] and cnt.tolist() == [2]
    # equal scores: the stable sort puts the lower index first, so of two identical boxes the first survives
    b = torch.tensor([[5.0, 5, 50, 50], [200, 200, 240, 260], [5, 5, 50, 50], [200, 200, 240, 260]])
    s = torch.tensor([0.5, 0.5, 0.5, 0.5])
    order = torch.sort(s, descending=True, stable=True).indices
    assert order.tolist() == [0, 1, 2, 3]
    rank, _ = ops.nms_segments(_t(b[order]), _t([0, 4], torch.int32), 0.5)
    assert rank.tolist() == [0, 1, -1, -1]
    # an invalid box is never kept and suppresses nothing
    rank, cnt = ops.nms_segments(_t(b), _t([0, 4], torch.int32), 0.5, _t([0, 1, 1, 1], torch.uint8))
    assert rank.tolist() == [-1, 0, 1, -1] and cnt.tolist() == [2]
    # offsets that do not describe a segment: nothing is kept there, the rest is untouched
    rank, cnt = ops.nms_segments(_t(b), _t([0, 2, 9], torch.int32), 0.5, max_seg=8)
    assert rank.tolist() == [0, 1, -1, -1] and cnt.tolist() == [2, 0]


# ------------------------------------------------------------------ decode
def _gate(ref32, ref64, floor):
    return max(2.0 * float(np.abs(np.asarray(ref32, np.float64) - ref64).max()), floor)


def test_rpn_decode():
    """flags equal; coordinates within 2 x the fp32 torch formulation's distance from fp64 (floor: one fp32 ulp at F,
    which covers an `exp` that differs in the last bit); scores likewise (floor: two fp32 ulps at 1)"""
    c = chk.rpn_decode_case(21)
    heads = [torch.from_numpy(h) for h in c["heads"]]
    idx = torch.from_numpy(c["idx"])
    rb, rs, rv = det.rpn_decode_torch(heads, c["grids"], c["k_off"], det.base_anchors(), idx, c["F"], c["min_size"],
                                      c["score_thresh"])
    assert np.array_equal(rv.numpy(), c["valid"])
    gate_b = _gate(rb.numpy(), c["boxes"], float(np.spacing(np.float32(c["F"]))))
    gate_s = _gate(rs.numpy(), c["scores"], 2.0 ** -22)
    boxes, scores, valid = ops.rpn_decode([h.to(DEV) for h in heads], c["grids"], c["k_off"], det.base_anchors(),
                                          idx.to(DEV), c["F"], c["min_size"], c["score_thresh"])
    assert np.array_equal(valid.cpu().numpy(), c["valid"])
    eb = float(np.abs(boxes.double().cpu().numpy() - c["boxes"]).max())
    es = float(np.abs(scores.double().cpu().numpy() - c["scores"]).max())
    print(f"rpn_decode: box err {eb:.3e} (gate {gate_b:.3e}), score err {es:.3e} (gate {gate_s:.3e})")
    assert eb <= gate_b and es <= gate_s
    # an index outside its level is never an address: a zero box, not valid
    bad = idx.clone()
    bad[0, 0], bad[1, -1] = -1, 10 ** 9
    boxes, _, valid = ops.rpn_decode([h.to(DEV) for h in heads], c["grids"], c["k_off"], det.base_anchors(),
                                     bad.to(DEV), c["F"], c["min_size"], c["score_thresh"])
    assert valid[0, 0] == 0 and valid[1, -1] == 0 and float(boxes[0, 0].abs().max()) == 0


def test_roi_decode():
    r = chk.roi_decode_case(22)
    out, props, C = torch.from_numpy(r["out"]), torch.from_numpy(r["props"]), r["C"]
    args = (r["weights"], r["W"], r["H"], r["min_size"], r["score_thresh"])
    rb, rs, rv = det.roi_decode_torch(props, out[:, :C], out[:, C:5 * C], *args)
    assert np.array_equal(rv.numpy(), r["valid"])
    gate_b = _gate(rb.numpy(), r["boxes"], float(np.spacing(np.float32(r["W"]))))
    gate_s = _gate(rs.numpy(), r["scores"], 2.0 ** -22)
    o = out.to(DEV)
    boxes, scores, valid = ops.roi_decode(props.to(DEV), o[:, :C], o[:, C:5 * C], *args)
    assert np.array_equal(valid.cpu().numpy(), r["valid"])
    eb = float(np.abs(boxes.double().cpu().numpy() - r["boxes"]).max())
    es = float(np.abs(scores.double().cpu().numpy() - r["scores"]).max())
    print(f"roi_decode: box err {eb:.3e} (gate {gate_b:.3e}), score err {es:.3e} (gate {gate_s:.3e})")
    assert eb <= gate_b and es <= gate_s


# ------------------------------------------------------------------ RoIAlign
@functools.lru_cache(maxsize=None)
def _roi_reference(C):
    """computed once per channel count: the case, the fp64 restatement with its autograd gradient, and the fp32 torch
    formulation's own distance from both"""
    maps, rois, roi_batch, _ = chk.roi_align_case(31, C)
    dy = torch.randn(37, C * 49, generator=torch.Generator().manual_seed(32))
    m64 = [m.double().requires_grad_(True) for m in maps]
    ref = chk.roi_align_ref(m64, chk.ROI_SCALES, rois, roi_batch)
    ref.backward(dy.double())
    m32 = [m.clone().requires_grad_(True) for m in maps]
    t32 = det.roi_align_torch(m32, chk.ROI_SCALES, rois, roi_batch)
    t32.backward(dy)
    d_fwd = float((t32.detach().double() - ref.detach()).abs().max())
    d_bwd = [float((a.grad.double() - b.grad).abs().max()) for a, b in zip(m32, m64)]
    return maps, rois, roi_batch, dy, ref.detach(), [m.grad for m in m64], d_fwd, d_bwd


def test_level_mapper():
    rois, exp = chk.level_case(33)
    maps = [torch.zeros(1, h, h, 64, device=DEV).permute(0, 3, 1, 2) for h in (64, 32, 16, 8)]
    _, lv = ops.roi_align_fwd(maps, (0.25, 0.125, 0.0625, 0.03125), _t(rois), _t(np.zeros(len(rois)), torch.int32),
                              torch.float32, want_levels=True)
    assert np.array_equal(lv.cpu().numpy(), exp)


@pytest.mark.parametrize("C", [64, 256])
def test_roi_align_fwd(C):
    """gate: 2 x the fp32 torch formulation's max distance from fp64 on the case (coordinate rounding times map slope
    dominates, and depends on the input), floor 2^-20 max|x|.  Measured reference distance on these cases: 6.9e-6 at
    C = 64 (max|x| 4.36), 7.3e-6 at C = 256 (max|x| 4.97); the floor would be 4.2e-6 / 4.7e-6."""
    maps, rois, roi_batch, _, ref, _, d_fwd, _ = _roi_reference(C)
    xmax = max(float(m.abs().max()) for m in maps)
    gate = max(2.0 * d_fwd, 2.0 ** -20 * xmax)
    out, lv = ops.roi_align_fwd([m.to(DEV) for m in maps], chk.ROI_SCALES, rois.to(DEV), roi_batch.to(DEV),
                                torch.float32, want_levels=True)
    assert np.array_equal(lv.cpu().numpy(), chk.levels_ref(rois.numpy()))
    err = float((out.double().cpu() - ref).abs().max())
    print(f"roi_align_fwd C={C}: err {err:.3e}, reference distance {d_fwd:.3e}, gate {gate:.3e}")
    assert out.shape == (37, C * 49) and err <= gate
    # bf16 output: the same values rounded once
    ob = ops.roi_align_fwd([m.to(DEV) for m in maps], chk.ROI_SCALES, rois.to(DEV), roi_batch.to(DEV), torch.bfloat16)
    assert torch.equal(ob, out.to(torch.bfloat16))
    # a RoI of an image that is not there gives zeros; other layouts are refused
    bad = roi_batch.clone()
    bad[3] = 7
    ob = ops.roi_align_fwd([m.to(DEV) for m in maps], chk.ROI_SCALES, rois.to(DEV), bad.to(DEV), torch.float32)
    assert float(ob[3].abs().max()) == 0 and torch.equal(ob[4], out[4])
    with pytest.raises(RuntimeError, match="channels-last"):
        ops.roi_align_fwd([m.to(DEV).contiguous() for m in maps], chk.ROI_SCALES, rois.to(DEV), roi_batch.to(DEV),
                          torch.float32)


@pytest.mark.parametrize("C", [64, 256])
def test_roi_align_bwd(C):
    """against fp64 autograd; gate per map: 2 x the fp32 torch formulation's gradient distance from fp64, floor
    2^-20 max|grad|"""
    maps, rois, roi_batch, dy, _, g64, _, d_bwd = _roi_reference(C)
    dm = [torch.zeros(m.shape[0], m.shape[2], m.shape[3], C, device=DEV).permute(0, 3, 1, 2) for m in maps]
    ops.roi_align_bwd(dm, chk.ROI_SCALES, rois.to(DEV), roi_batch.to(DEV), dy.to(DEV))
    for l in range(4):
        gate = max(2.0 * d_bwd[l], 2.0 ** -20 * float(g64[l].abs().max()))
        err = float((dm[l].double().cpu() - g64[l]).abs().max())
        print(f"roi_align_bwd C={C} level {l}: err {err:.3e}, reference distance {d_bwd[l]:.3e}, gate {gate:.3e}")
        assert err <= gate


def test_roi_align_bwd_bf16_dy():
    """the bf16 operand path of the backward: dy in bf16, against fp64 autograd of the same (rounded) dy; the gate in the
    same form, from the fp32 torch formulation's gradient error.  The fp64 reference here is the torch formulation run
    in fp64, which the CPU tests hold to the sample-by-sample restatement."""
    C = 64
    maps, rois, roi_batch, dy, _, _, _, _ = _roi_reference(C)
    dyb = dy.to(torch.bfloat16)
    m64 = [m.double().requires_grad_(True) for m in maps]
    det.roi_align_torch(m64, chk.ROI_SCALES, rois.double(), roi_batch).backward(dyb.double())
    m32 = [m.clone().requires_grad_(True) for m in maps]
    det.roi_align_torch(m32, chk.ROI_SCALES, rois, roi_batch).backward(dyb.float())
    dm = [torch.zeros(m.shape[0], m.shape[2], m.shape[3], C, device=DEV).permute(0, 3, 1, 2) for m in maps]
    ops.roi_align_bwd(dm, chk.ROI_SCALES, rois.to(DEV), roi_batch.to(DEV), dyb.to(DEV))
    for l in range(4):
        d = float((m32[l].grad.double() - m64[l].grad).abs().max())
        gate = max(2.0 * d, 2.0 ** -20 * float(m64[l].grad.abs().max()))
        err = float((dm[l].double().cpu() - m64[l].grad).abs().max())
        print(f"roi_align_bwd bf16 dy level {l}: err {err:.3e}, gate {gate:.3e}")
        assert err <= gate


def test_roi_align_bwd_colliding_adds():
    """64 identical RoIs: every add lands on the same rows.  The gate of one RoI, scaled by the count.  Measured on
    level 0 (the only one the RoI maps to): err 1.30e-4 against a gate of 2.11e-4, as 64 sequential fp32 adds of the one
    RoI's gradient give on the host; a backward that adds tap by tap (about 350 adds per element) measured 2.75e-4."""
    C, n = 64, 64
    g = torch.Generator().manual_seed(41)
    maps = [torch.randn(1, h, h, C, generator=g).permute(0, 3, 1, 2) for h in chk.ROI_GRIDS]
    roi = torch.tensor([[13.3, 21.7, 61.2, 70.9]])
    rb = torch.zeros(1, dtype=torch.int32)
    dy = torch.randn(1, C * 49, generator=g)
    m64 = [m.double().requires_grad_(True) for m in maps]
    chk.roi_align_ref(m64, chk.ROI_SCALES, roi, rb).backward(dy.double())
    m32 = [m.clone().requires_grad_(True) for m in maps]
    det.roi_align_torch(m32, chk.ROI_SCALES, roi, rb).backward(dy)
    dm = [torch.zeros(1, h, h, C, device=DEV).permute(0, 3, 1, 2) for h in chk.ROI_GRIDS]
    ops.roi_align_bwd(dm, chk.ROI_SCALES, roi.repeat(n, 1).to(DEV), rb.repeat(n).to(DEV), dy.repeat(n, 1).to(DEV))
    for l in range(4):
        if m64[l].grad is None:   # the RoI maps to one level: the others receive nothing
            assert l != 0 and float(dm[l].abs().max()) == 0
            continue
        want = n * m64[l].grad
        d = float((m32[l].grad.double() - m64[l].grad).abs().max())
        gate = n * max(2.0 * d, 2.0 ** -20 * float(m64[l].grad.abs().max()))
        err = float((dm[l].double().cpu() - want).abs().max())
        print(f"colliding adds level {l}: err {err:.3e}, gate {gate:.3e}")
        assert err <= gate and float(dm[l].abs().max()) > 0


# ------------------------------------------------------------------ model
F = 256


class _FixedSample(det.FasterRCNN):
    """the sampler fixed through the override: fixed keys (a multiplicative hash of the index, so that the sample spreads
    over every level) instead of a random draw"""

    @staticmethod
    def _keys(labels):
        i = torch.arange(labels.shape[0], device=labels.device, dtype=torch.int64)
        return ((i * 2654435761) % 4294967296).double().div(4294967296.0).float()

    def sample_rpn(self, labels):
        return det.balanced_sample(labels, *self.cfg["rpn_sample"], keys=self._keys(labels))

    def sample_roi(self, labels):
        return det.balanced_sample(labels, *self.cfg["box_sample"], keys=self._keys(labels))


def _model(prec="fp32", seed=0, cls=chk.recording(_FixedSample), num_classes=2):
    from ssl4gie_amd.Models import models
    torch.manual_seed(seed)
    backbone = models.VisionTransformer_from_Any(False, 0, False, None, True, F, 768, 12, 12, "cls")
    m = cls(backbone, num_classes=num_classes, image_mean=[0.485, 0.456, 0.406], image_std=[0.229, 0.224, 0.225])
    m.transform.fixed_size = (F, F)
    with torch.no_grad():   # heads that decide something: the reference's 0.01 initialisation leaves every score at 0.5
        g = torch.Generator().manual_seed(seed + 1)
        for p in list(m.rpn.parameters()) + list(m.roi_heads.box_predictor.parameters()):
            p.copy_(torch.randn(p.shape, generator=g) * (0.05 if p.dim() > 1 else 0.2))
    return m.to(DEV).set_precision(prec)


def _batch(seed=5, B=2):
    g = torch.Generator().manual_seed(seed)
    images = torch.rand(B, 3, F, F, generator=g).to(DEV)
    targets = []
    for b in range(B):
        k = 1 + (b + seed) % 3
        x1, y1 = torch.rand(k, generator=g) * 120 + 10, torch.rand(k, generator=g) * 120 + 10
        w, h = torch.rand(k, generator=g) * 90 + 25, torch.rand(k, generator=g) * 90 + 25
        targets.append({"boxes": torch.stack([x1, y1, x1 + w, y1 + h], 1).to(DEV),
                        "labels": torch.ones(k, dtype=torch.int64, device=DEV)})
    return list(images.unbind(0)), targets


def test_stagewise_parity_eval(monkeypatch):
    """every stage's kernel against the torch formulation fed with the ENGINE's upstream outputs, so that a decision
    flipped upstream cannot cascade: proposals (candidates decoded, NMS), pooled features, final detections"""
    m = _model().eval()
    images, _ = _batch()
    with torch.no_grad():
        res = m(images)
    L = m.last
    heads, grids, B = [h.float() for h in L["heads"]], L["grids"], 2
    # proposals: decode (gate: 2 x the fp32 torch formulation's distance from the same formulation in fp64)
    idx, k_off = m.rpn_candidates(heads, grids, B)
    base = det.base_anchors()
    boxes, scores, valid = ops.rpn_decode(heads, grids, k_off, base, idx, F, 1e-3, 0.0)
    tb, ts, tv = det.rpn_decode_torch(heads, grids, k_off, base, idx, F, 1e-3, 0.0)
    db_, ds_, _ = det.rpn_decode_torch([h.double() for h in heads], grids, k_off, base, idx, F, 1e-3, 0.0)
    assert torch.equal(valid, tv)
    ulp = float(np.spacing(np.float32(F)))
    assert float((boxes.double() - db_).abs().max()) <= max(2 * float((tb.double() - db_).abs().max()), ulp)
    assert float((scores.double() - ds_).abs().max()) <= max(2 * float((ts.double() - ds_).abs().max()), 2.0 ** -22)
    # proposals: NMS on the engine's boxes -> equal index sets; the selection behind it is shared
    seg, max_seg = m.rpn_segments(B, k_off, DEV)
    kr, kc = ops.nms_segments(boxes.view(-1, 4), seg, 0.7, valid.view(-1), max_seg)
    tr, tc = det.nms_segments_torch(boxes.view(-1, 4), seg, 0.7, valid.view(-1), max_seg)
    assert torch.equal(kr, tr) and torch.equal(kc, tc) and int(kc.sum()) > 0 and int((kr < 0).sum()) > 0
    props, ok = L["props"], L["ok"]
    assert ok.sum(1).tolist() == [min(int(c), 1000) for c in kc.view(B, -1).sum(1)]
    # ... and the whole proposal stage as torch ops on the engine's heads: the same proposals in the same order
    gate_b = max(2 * float((tb.double() - db_).abs().max()), ulp)
    monkeypatch.setenv("SSL4GIE_FUSED_DET_HEADS", "0")
    tprops, tok, _ = m.rpn_proposals(heads, grids, B, F)
    monkeypatch.delenv("SSL4GIE_FUSED_DET_HEADS")
    assert torch.equal(tok, ok) and float((tprops - props).abs().max()) <= 2 * gate_b
    # pooled features of the first 48 proposals of every image
    maps = [L["features"][k] for k in ("0", "1", "2", "3")]
    scales = [2.0 ** round(math.log2(x.shape[2] / F)) for x in maps]
    rois = props[:, :48].reshape(-1, 4).contiguous()
    rb = torch.arange(B, dtype=torch.int32, device=DEV).repeat_interleave(48)
    pooled = ops.roi_align_fwd(maps, scales, rois, rb, torch.float32)
    p32 = det.roi_align_torch(maps, scales, rois, rb)
    p64 = det.roi_align_torch([x.double() for x in maps], scales, rois.double(), rb)
    gate = max(2.0 * float((p32.double() - p64).abs().max()), 2.0 ** -20 * max(float(x.abs().max()) for x in maps))
    assert float((pooled.double() - p64).abs().max()) <= gate
    # final detections: decode on the engine's head outputs, per-class NMS on the engine's sorted boxes
    out, C = L["out"].float(), m.num_classes
    pf = props.reshape(-1, 4).contiguous()
    args = ((10.0, 10.0, 5.0, 5.0), F, F, 1e-2, 0.05)
    eb, es, ev = ops.roi_decode(pf, out[:, :C], out[:, C:5 * C], *args)
    tb, ts, tv = det.roi_decode_torch(pf, out[:, :C], out[:, C:5 * C], *args)
    db_, ds_, _ = det.roi_decode_torch(pf.double(), out[:, :C].double(), out[:, C:5 * C].double(), *args)
    assert torch.equal(ev, tv)
    assert float((eb.double() - db_).abs().max()) <= max(2 * float((tb.double() - db_).abs().max()), ulp)
    assert float((es.double() - ds_).abs().max()) <= max(2 * float((ts.double() - ds_).abs().max()), 2.0 ** -22)
    bs, ss, vs = m.box_candidates(out, props, ok, F)
    P = ok.shape[1]
    seg = torch.arange(0, (B * (C - 1) + 1) * P, P, dtype=torch.int32, device=DEV)
    kr, kc = ops.nms_segments(bs.view(-1, 4), seg, 0.5, vs.view(-1), P)
    tr, tc = det.nms_segments_torch(bs.view(-1, 4), seg, 0.5, vs.view(-1), P)
    assert torch.equal(kr, tr) and torch.equal(kc, tc) and int(kc.sum()) > 0
    _, _, _, cnt = m.postprocess(out, props, ok, F)
    assert cnt.tolist() == [min(int(c), 100) for c in kc.view(B, -1).sum(1)] == [len(r["boxes"]) for r in res]
    _final_detections_match(m, monkeypatch, res, out, props, ok)


def _final_detections_match(m, monkeypatch, res, out, props, ok):
    """what forward returned against (1) the whole final stage as torch ops on the engine's head outputs — boxes and
    scores within twice the decode gate (either side may sit a gate away from fp64), labels and order equal — and (2),
    detection by detection, the torch decode of that detection's class: the box of class `label` of some proposal of the
    image, with that class's softmax score"""
    C, (B, P) = m.num_classes, ok.shape
    pf = props.reshape(-1, 4).contiguous()
    args = ((10.0, 10.0, 5.0, 5.0), F, F, 1e-2, 0.05)
    tb, ts, _ = det.roi_decode_torch(pf, out[:, :C], out[:, C:5 * C], *args)
    db_, ds_, _ = det.roi_decode_torch(pf.double(), out[:, :C].double(), out[:, C:5 * C].double(), *args)
    gate_b = max(2 * float((tb.double() - db_).abs().max()), float(np.spacing(np.float32(F))))
    gate_s = max(2 * float((ts.double() - ds_).abs().max()), 2.0 ** -22)
    monkeypatch.setenv("SSL4GIE_FUSED_DET_HEADS", "0")
    tdb, tds, tdl, tcnt = m.postprocess(out, props, ok, F)
    monkeypatch.delenv("SSL4GIE_FUSED_DET_HEADS")
    tb, ts = tb.view(B, P, C - 1, 4), ts.view(B, P, C - 1)
    for b, r in enumerate(res):
        n = int(tcnt[b])
        assert len(r["boxes"]) == n
        assert torch.equal(r["labels"], tdl[b, :n])
        assert float((r["boxes"] - tdb[b, :n]).abs().max()) <= 2 * gate_b
        assert float((r["scores"] - tds[b, :n]).abs().max()) <= 2 * gate_s
        for box, lab, sc in zip(r["boxes"], r["labels"], r["scores"]):
            c = int(lab) - 1
            hit = ((tb[b, :, c] - box).abs().amax(1) <= 2 * gate_b) & ((ts[b, :, c] - sc).abs() <= 2 * gate_s) & ok[b]
            assert bool(hit.any()), (b, int(lab))


def test_final_detections_with_several_classes(monkeypatch):
    """num_classes = 4, so that the class of a detection (segment index -> label, the per-class delta columns) can be
    wrong: forward's detections against the torch formulation of the final stage"""
    m = _model(num_classes=4, seed=3).eval()
    images, _ = _batch(seed=6)
    with torch.no_grad():
        res = m(images)
    L = m.last
    labels = torch.cat([r["labels"] for r in res])
    assert labels.numel() > 0 and int(labels.min()) >= 1 and int(labels.max()) <= 3 and labels.unique().numel() >= 2
    _final_detections_match(m, monkeypatch, res, L["out"].float(), L["props"], L["ok"])


def test_eval_structure_and_map():
    """at most 100 detections per image, scores descending and >= 0.05, labels in [1, C), boxes inside the image; the
    output goes through MeanAveragePrecision.update / compute unchanged"""
    from ssl4gie_amd.metrics import MeanAveragePrecision
    m = _model().eval()
    images, targets = _batch()
    with torch.no_grad():
        out = m(images)
    assert isinstance(out, list) and len(out) == 2
    n = 0
    for r in out:
        assert set(r) == {"boxes", "labels", "scores"}
        k = r["boxes"].shape[0]
        n += k
        assert k <= 100 and r["boxes"].shape == (k, 4) and r["labels"].dtype == torch.int64
        if k:
            assert bool((r["scores"][:-1] >= r["scores"][1:]).all()) and float(r["scores"].min()) >= 0.05
            assert int(r["labels"].min()) >= 1 and int(r["labels"].max()) < 2
            assert float(r["boxes"].min()) >= 0 and float(r["boxes"].max()) <= F
            assert bool((r["boxes"][:, 2] >= r["boxes"][:, 0]).all())
    assert n > 0
    metric = MeanAveragePrecision()
    metric.update(out, targets)
    res = metric.compute()
    assert 0.0 <= float(res["map"]) <= 1.0


def _torchvision_losses(m):
    """torchvision's compute_loss / fastrcnn_loss with index tensors, on the engine's head outputs"""
    import torch.nn.functional as Fn
    r, L = m.last["rpn"], m.last
    pos = torch.where(r["pos"].reshape(-1))[0]
    sel = torch.where(r["sampled"].reshape(-1))[0]
    logits, deltas = r["logits"].reshape(-1).float(), r["deltas"].reshape(-1, 4).float()
    labels, reg = r["labels"].reshape(-1), r["reg"].reshape(-1, 4)
    box = Fn.smooth_l1_loss(deltas[pos], reg[pos], beta=1 / 9, reduction="sum") / sel.numel()
    obj = Fn.binary_cross_entropy_with_logits(logits[sel], labels[sel])
    C = m.num_classes
    out = L["out"].float()
    sv = torch.where(L["sampled"].reshape(-1))[0]
    cl, br = out[sv, :C], out[sv, C:5 * C]
    lab, rt = L["labels"].reshape(-1)[sv], L["reg"].reshape(-1, 4)[sv]
    ce = Fn.cross_entropy(cl, lab)
    p = torch.where(lab > 0)[0]
    bl = Fn.smooth_l1_loss(br.reshape(-1, C, 4)[p, lab[p]], rt[p], beta=1 / 9, reduction="sum") / lab.numel()
    return {"loss_classifier": ce, "loss_box_reg": bl, "loss_objectness": obj, "loss_rpn_box_reg": box}


def test_training_losses_and_gradients():
    m = _model().train()
    images, targets = _batch()
    losses = m(images, targets)
    assert list(losses) == ["loss_classifier", "loss_box_reg", "loss_objectness", "loss_rpn_box_reg"]
    ref = _torchvision_losses(m)
    for k, v in losses.items():
        v = v.detach()
        assert math.isfinite(float(v)) and float(v) > 0, k
        assert abs(float(v) - float(ref[k])) <= 1e-5 * abs(float(ref[k])), (k, float(v), float(ref[k]))
    assert int(m.last["sampled"].sum()) > 0 and int((m.last["labels"] > 0).sum()) > 0 and int(m.last["rpn"]["pos"].sum()) > 0
    sum(losses.values()).backward()
    for name, p in m.named_parameters():
        if not p.requires_grad:
            continue
        assert p.grad is not None, name
        assert bool(torch.isfinite(p.grad).all()) and float(p.grad.abs().max()) > 0, name


def test_learning_check_on_one_batch():
    """20 ArenaAdamW steps on one fixed batch with the sampler fixed: the summed loss ends below the first step's"""
    from ssl4gie_amd.optim import ArenaAdamW
    m = _model().train()
    opt = ArenaAdamW(m, [p for p in m.parameters() if p.requires_grad], lr=1e-4, weight_decay=0.0)
    images, targets = _batch()
    first = last = None
    for step in range(20):
        opt.zero_grad()
        loss = sum(m(images, targets).values())
        loss.backward()
        opt.step()
        last = float(loss.detach())
        first = last if first is None else first
        assert math.isfinite(last)
    print(f"learning check: {first:.4f} -> {last:.4f}")
    assert last < first


def test_bf16_forward_backward_runs():
    m = _model("bf16", cls=det.FasterRCNN).train()
    images, targets = _batch()
    losses = m(images, targets)
    sum(losses.values()).backward()
    assert all(math.isfinite(float(v.detach())) for v in losses.values())
    assert all(bool(torch.isfinite(p.grad).all()) for p in m.parameters() if p.grad is not None)
    m.eval()
    with torch.no_grad():
        out = m(images)
    assert len(out) == 2


def test_reference_loop_statements_on_detection_loader_batches():
    """train_detection.py:67-81 and :118-123 verbatim (rank 0, one process) on DetectionLoader batches"""
    from ssl4gie_amd.data import DetectionLoader, DetectionTransform, RaggedImageBank
    from ssl4gie_amd.metrics import MeanAveragePrecision
    from ssl4gie_amd.optim import ArenaAdamW
    rng = np.random.default_rng(3)
    imgs = [rng.integers(0, 255, (200 + 8 * i, 240 - 4 * i, 3), dtype=np.uint8) for i in range(4)]
    bxs = [np.array([[20.0 + i, 30, 120, 150 + i]], dtype=np.float32) for i in range(4)]
    bank = RaggedImageBank.from_arrays(imgs, bxs, DEV, box_labels=np.ones(4, dtype=np.int64))
    train_loader = DetectionLoader(bank, 2, sampler=torch.utils.data.SequentialSampler(bank),
                                   transform=DetectionTransform(F, generator=torch.Generator(device=DEV).manual_seed(1)))
    test_loader = DetectionLoader(bank, 2, sampler=torch.utils.data.SequentialSampler(bank),
                                  transform=DetectionTransform.eval(F))
    model = _model(cls=det.FasterRCNN)
    optimizer = ArenaAdamW(model, [p for p in model.parameters() if p.requires_grad], lr=1e-5)
    scaler = torch.cuda.amp.GradScaler(enabled=False)
    rank, accum_iter = 0, 1
    model.train()
    loss_accumulator = []
    optimizer.zero_grad()
    for batch_idx, (data, target) in enumerate(train_loader):
        data = list(image.cuda(rank) for image in data)
        target = [{k: v.cuda(rank) for k, v in t.items()} for t in target]

        with torch.cuda.amp.autocast():
            loss_dict = model(data, target)
            loss = sum(loss for loss in loss_dict.values()) / accum_iter
        loss_accumulator.append(loss.item())
        scaler.scale(loss).backward()
        if (batch_idx + 1) % accum_iter == 0:
            scaler.step(optimizer)
            scaler.update()
            optimizer.zero_grad()
    assert len(loss_accumulator) == 2 and all(math.isfinite(v) for v in loss_accumulator)
    metric = MeanAveragePrecision()
    model.eval()
    N = 0
    with torch.no_grad():
        for batch_idx, (data, target) in enumerate(test_loader):
            data = list(image.cuda(rank) for image in data)
            target = [{k: v.cuda(rank) for k, v in t.items()} for t in target]
            N += len(data)
            output = model(data)
            metric.update(output, target)
    metric_dict = metric.compute()
    assert N == 4 and math.isfinite(metric_dict["map"].item())
