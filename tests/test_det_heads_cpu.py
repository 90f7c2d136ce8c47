"""CPU: the fp64 restatements of tests/det_head_checks.py agree with the torch formulations of
ssl4gie_amd/Models/detection.py (the kernels' fp32 reference and fallback), the anchor rule, the detector's state_dict
schema, and the refusals (segment cap, transform)."""
import numpy as np
import pytest
import torch

import det_head_checks as chk
from ssl4gie_amd import ops
from ssl4gie_amd.Models import detection as det


def test_nms_restatement_agrees_with_torch_formulation():
    for thr, sizes, seed in ((0.7, (1, 63, 0, 64, 65, 257), 1), (0.5, (130, 2, 40), 2)):
        boxes, seg_off, valid = chk.nms_case(sizes, thr, seed)
        rank, cnt = chk.nms_ref(boxes, seg_off, thr, valid)
        r2, c2 = det.nms_segments_torch(torch.from_numpy(boxes), torch.from_numpy(seg_off), thr, torch.from_numpy(valid))
        assert np.array_equal(rank, r2.numpy()) and np.array_equal(cnt, c2.numpy())
    boxes, seg_off = chk.nms_exact_case()
    for thr, want in ((0.5, [0, 1, 0, -1]), (0.7, [0, 1, 0, 1])):
        assert chk.nms_ref(boxes, seg_off, thr)[0].tolist() == want
        assert det.nms_segments_torch(torch.from_numpy(boxes), torch.from_numpy(seg_off), thr)[0].tolist() == want
    boxes, seg_off = chk.nms_chain_case()
    assert chk.nms_ref(boxes, seg_off, 0.5)[0].tolist() == [0, -1, 1]
    assert det.nms_segments_torch(torch.from_numpy(boxes), torch.from_numpy(seg_off), 0.5)[0].tolist() == [0, -1, 1]


def test_anchor_rule():
    """count 3 * sum(grid^2) and the first and last box of every level at F = 256 (torchvision's AnchorGenerator:
    sizes 32 .. 512, ratios 0.5 / 1 / 2, base round([-w, -h, w, h] / 2), stride = image // grid, anchor fastest)"""
    F = 256
    grids = [64, 32, 16, 8, 4]
    base = det.base_anchors()
    assert np.array_equal(base.numpy(), chk.base_anchors_ref())
    assert base[0].tolist() == [[-23, -11, 23, 11], [-16, -16, 16, 16], [-11, -23, 11, 23]]
    assert base[4].tolist() == [[-362, -181, 362, 181], [-256, -256, 256, 256], [-181, -362, 181, 362]]
    anchors = det.grid_anchors(base, grids, F)
    assert sum(a.shape[0] for a in anchors) == 3 * sum(g * g for g in grids) == 16368
    assert 3 * sum(g * g for g in (256, 128, 64, 32, 16)) == 261888
    first = [[-23, -11, 23, 11], [-45, -23, 45, 23], [-91, -45, 91, 45], [-181, -91, 181, 91], [-362, -181, 362, 181]]
    for l, (a, g) in enumerate(zip(anchors, grids)):
        s = F // g
        assert a[0].tolist() == first[l]
        last = base[l, 2] + torch.tensor([(g - 1) * s, (g - 1) * s, (g - 1) * s, (g - 1) * s], dtype=torch.float32)
        assert a[-1].tolist() == last.tolist()
        for flat in (0, 1, 3 * g + 2, 3 * g * g - 1):
            assert a[flat].tolist() == chk.anchor_ref(l, g, F, flat).tolist()


def test_decode_restatements_agree_with_torch_formulations():
    c = chk.rpn_decode_case(3)
    heads = [torch.from_numpy(h) for h in c["heads"]]
    boxes, scores, valid = det.rpn_decode_torch(heads, c["grids"], c["k_off"], det.base_anchors(),
                                                torch.from_numpy(c["idx"]), c["F"], c["min_size"], c["score_thresh"])
    assert np.array_equal(valid.numpy(), c["valid"])
    assert np.abs(boxes.double().numpy() - c["boxes"]).max() < 1e-3 and np.abs(scores.double().numpy() - c["scores"]).max() < 1e-6
    r = chk.roi_decode_case(4)
    out = torch.from_numpy(r["out"])
    C = r["C"]
    boxes, scores, valid = det.roi_decode_torch(torch.from_numpy(r["props"]), out[:, :C], out[:, C:5 * C], r["weights"],
                                                r["W"], r["H"], r["min_size"], r["score_thresh"])
    assert np.array_equal(valid.numpy(), r["valid"])
    assert np.abs(boxes.double().numpy() - r["boxes"]).max() < 1e-3 and np.abs(scores.double().numpy() - r["scores"]).max() < 1e-6


def test_level_mapper_restatement_agrees_with_torch_formulation():
    rois, exp = chk.level_case(5)
    assert np.array_equal(det.roi_levels_torch(torch.from_numpy(rois)).numpy(), exp)


def test_roi_align_restatement_agrees_with_torch_formulation():
    maps, rois, roi_batch, _ = chk.roi_align_case(6, 64)
    m64 = [m.double().requires_grad_(True) for m in maps]
    ref = chk.roi_align_ref(m64, chk.ROI_SCALES, rois, roi_batch)
    n64 = [m.double().requires_grad_(True) for m in maps]
    got = det.roi_align_torch(n64, chk.ROI_SCALES, rois.double(), roi_batch)
    assert got.shape == ref.shape == (37, 64 * 49)
    assert (got - ref).abs().max() < 1e-12
    dy = torch.randn(ref.shape, dtype=torch.float64, generator=torch.Generator().manual_seed(7))
    ref.backward(dy)
    got.backward(dy)
    for a, b in zip(m64, n64):
        assert (a.grad - b.grad).abs().max() < 1e-11


class _Backbone(torch.nn.Module):
    out_channels = 256

    def __init__(self):
        super().__init__()
        self.body = torch.nn.Conv2d(3, 8, 1)


@pytest.mark.parametrize("num_classes", [2, 91])
def test_state_dict_schema(num_classes):
    m = det.FasterRCNN(_Backbone(), num_classes=num_classes, image_mean=[0.485, 0.456, 0.406],
                       image_std=[0.229, 0.224, 0.225])
    sd = m.state_dict()
    want = {"rpn.head.conv.weight": (256, 256, 3, 3), "rpn.head.conv.bias": (256,),
            "rpn.head.cls_logits.weight": (3, 256, 1, 1), "rpn.head.cls_logits.bias": (3,),
            "rpn.head.bbox_pred.weight": (12, 256, 1, 1), "rpn.head.bbox_pred.bias": (12,),
            "roi_heads.box_head.fc6.weight": (1024, 12544), "roi_heads.box_head.fc6.bias": (1024,),
            "roi_heads.box_head.fc7.weight": (1024, 1024), "roi_heads.box_head.fc7.bias": (1024,),
            "roi_heads.box_predictor.cls_score.weight": (num_classes, 1024),
            "roi_heads.box_predictor.cls_score.bias": (num_classes,),
            "roi_heads.box_predictor.bbox_pred.weight": (4 * num_classes, 1024),
            "roi_heads.box_predictor.bbox_pred.bias": (4 * num_classes,)}
    heads = {k: tuple(v.shape) for k, v in sd.items() if not k.startswith("backbone.")}
    assert heads == want
    assert {k for k in sd if k.startswith("backbone.")} == {"backbone.body.weight", "backbone.body.bias"}
    assert not list(m.buffers())
    assert float(m.rpn.head.conv.bias.detach().abs().max()) == 0 and 0.008 < float(m.rpn.head.conv.weight.detach().std()) < 0.012


def test_nms_refuses_more_than_4096_boxes_per_segment():
    boxes = torch.zeros(4097, 4)
    seg = torch.tensor([0, 4097], dtype=torch.int32)
    with pytest.raises(ValueError, match="4096"):
        ops.nms_segments(boxes, seg, 0.5)
    with pytest.raises(ValueError, match="4096"):
        ops.nms_segments(boxes, seg, 0.5, max_seg=4097)
    with pytest.raises(ValueError, match="4096"):
        det.nms_segments_torch(boxes, seg, 0.5)


def test_transform_refusals_and_batch_views():
    m = det.FasterRCNN(_Backbone(), num_classes=2)
    imgs = [torch.zeros(3, 64, 64), torch.zeros(3, 64, 64)]
    with pytest.raises(NotImplementedError):
        m.transform(imgs)                       # fixed_size not set: the transform does not resize
    m.transform.fixed_size = (64, 64)
    assert m.transform(imgs).shape == (2, 3, 64, 64)
    with pytest.raises(NotImplementedError):
        m.transform([torch.zeros(3, 64, 48)])
    with pytest.raises(NotImplementedError):
        m.transform([torch.zeros(3, 64, 64), torch.zeros(3, 32, 32)])
    m.transform.fixed_size = (64, 48)
    with pytest.raises(NotImplementedError):
        m.transform([torch.zeros(3, 64, 48)])   # square only
    m.transform.fixed_size = (64, 64)
    batch = torch.rand(3, 3, 64, 64)
    assert m.transform.batch(list(batch)).data_ptr() == batch.data_ptr()   # views of one batch are not copied
    x = m.transform(list(batch))
    mean = torch.tensor([0.485, 0.456, 0.406])[None, :, None, None]
    std = torch.tensor([0.229, 0.224, 0.225])[None, :, None, None]
    assert torch.equal(x, (batch - mean) / std)
    m.train()
    with pytest.raises(ValueError, match="targets"):
        m(list(batch))
