"""CPU: the detection metric.  tests/det_map_checks.py's fp64 restatement (pycocotools' loop order) and the torch
formulation of ssl4gie_amd.metrics.MeanAveragePrecision reproduce the example of torchmetrics' docstring — the one
published datum behind this unpinned boundary — and hand cases whose values were computed with the restatement; the
two agree on random cases; the interface refuses what is not built; the C ABI declares, binds and exports the
det_map entry points, with the arguments they refuse before any launch."""
import os
import re

import numpy as np
import pytest
import torch

import det_map_checks as dc
from conftest import ROOT

NEW_SYMBOLS = ("ssl4gie_det_map_workspace_bytes", "ssl4gie_det_map_match", "ssl4gie_det_map_order",
               "ssl4gie_det_map_accumulate")
SIX = float(torch.tensor(0.6))   # 0.6 rounded to fp32


def _metric(case, splits=1):
    from ssl4gie_amd import metrics
    m = metrics.MeanAveragePrecision()
    preds, target = dc.to_updates(case)
    step = max(1, -(-len(preds) // splits))
    for s in range(0, len(preds), step):
        m.update(preds[s:s + step], target[s:s + step])
    return m


def _both(case):
    """the restatement's summaries and the torch path's, after checking that they agree"""
    want, classes = dc.restate(case)
    m = _metric(case)
    f64, res = m.compute_f64(), m.compute()
    for k in dc.NAMES:
        assert f64[k].dtype == torch.float64 and f64[k].dim() == 0
        assert abs(float(f64[k]) - want[k]) <= 1e-9, (k, float(f64[k]), want[k])
        assert res[k].dtype == torch.float32 and res[k].dim() == 0
        assert float(res[k]) == float(f64[k].float()), k
    assert res["classes"].dtype == torch.int32 and res["classes"].tolist() == classes
    assert float(res["map_per_class"]) == -1.0 and float(res["mar_100_per_class"]) == -1.0
    assert set(res) == set(dc.NAMES) | {"map_per_class", "mar_100_per_class", "classes"}
    return want, res


def test_docstring_example_of_torchmetrics():
    want, res = _both(dc.docstring_case())
    expect = {"map": 0.6, "map_50": 1.0, "map_75": 1.0, "map_small": -1.0, "map_medium": -1.0, "map_large": 0.6,
              "mar_1": 0.6, "mar_10": 0.6, "mar_100": 0.6, "mar_small": -1.0, "mar_medium": -1.0, "mar_large": 0.6}
    for k, v in expect.items():
        assert abs(want[k] - v) < 1e-12, (k, want[k])
        assert float(res[k]) == float(torch.tensor(v)), (k, float(res[k]))     # the fp32 tensor torchmetrics prints
    assert float(res["map"]) == SIX


def test_a_miss_scored_above_a_hit():
    case = [dc.image([[300, 300, 400, 400], [0, 0, 100, 100]], [0.9, 0.8], [0, 0], [[0, 0, 100, 100]], [0])]
    want, _ = _both(case)
    assert want["map"] == want["map_50"] == want["map_75"] == want["map_large"] == pytest.approx(0.5, abs=1e-12)
    assert want["mar_1"] == 0.0 and want["mar_10"] == 1.0 and want["mar_100"] == 1.0
    assert want["map_small"] == -1.0 and want["map_medium"] == -1.0


def test_two_perfect_detections_on_a_medium_and_a_large_box():
    boxes = [[10, 10, 60, 60], [100, 100, 300, 300]]
    want, _ = _both([dc.image(boxes, [0.9, 0.8], [0, 0], boxes, [0, 0])])
    assert want["map"] == pytest.approx(1.0, abs=1e-12) and want["mar_1"] == 0.5 and want["mar_10"] == 1.0
    assert want["map_small"] == -1.0
    assert want["map_medium"] == pytest.approx(1.0, abs=1e-12) and want["map_large"] == pytest.approx(1.0, abs=1e-12)


def test_a_class_only_predicted_is_excluded_and_one_only_annotated_scores_zero():
    small, large = [10, 10, 60, 60], [100, 100, 300, 300]
    case = [dc.image([small, large], [0.9, 0.8], [1, 2], [small, large], [1, 3])]
    want, res = _both(case)
    assert res["classes"].tolist() == [1, 2, 3]
    assert want["map"] == pytest.approx(0.5, abs=1e-12)            # class 1: 1, class 3: 0, class 2: -1 and left out
    assert want["map_large"] == 0.0 and want["map_medium"] == pytest.approx(1.0, abs=1e-12)
    assert want["map_small"] == -1.0


def test_a_detection_over_an_ignored_and_a_regular_ground_truth():
    """In the range `medium` the 200^2 box is ignored and sorted behind the 50^2 one.  A detection that reaches the
    regular box takes it and never looks at the ignored one; a detection that reaches only the ignored box is matched
    to it and ignored itself: neither a true nor a false positive.  (IoU 0.8 lies below the seventh threshold, the
    fp32 value 0.800000011920929.)"""
    det = [10, 10, 50, 60]                        # 40 x 50 inside both boxes
    case = [dc.image([det], [0.9], [0], [[10, 10, 210, 210], [10, 10, 60, 60]], [0, 0])]
    e = dc.evaluate_img(case[0], 0, 2)
    assert e["g_ig"].tolist() == [False, True]
    assert e["ious"][0].tolist() == [pytest.approx(0.8), pytest.approx(0.05)]
    assert e["dtm"][:, 0].tolist() == [True] * 6 + [False] * 4      # 0.8 reaches 0.5 .. 0.75
    assert e["dt_ig"][:, 0].tolist() == [False] * 10                # unmatched, area 2000 inside the range
    det = [10, 10, 170, 210]                      # 160 x 200: IoU 0.8 with the large box, 2500 / 32000 with the small
    case = [dc.image([det], [0.9], [0], [[10, 10, 210, 210], [10, 10, 60, 60]], [0, 0])]
    e = dc.evaluate_img(case[0], 0, 2)
    assert e["dtm"][:, 0].tolist() == [True] * 6 + [False] * 4 and e["dt_ig"][:, 0].tolist() == [True] * 10
    want, _ = _both(case)
    assert want["map_medium"] == 0.0 and want["mar_medium"] == 0.0   # the one regular box is never found
    assert want["map_large"] == pytest.approx(0.6, abs=1e-12)


def test_only_the_first_hundred_detections_of_an_image_count():
    gt = [100, 100, 200, 200]
    misses = [[300 + i, 300, 340 + i, 340] for i in range(129)]
    scores = np.linspace(0.99, 0.2, 129).tolist()
    late = dc.image(misses + [gt], scores + [0.1], [0] * 130, [gt], [0])          # the hit has rank 129: dropped
    want, _ = _both([late])
    assert want["map"] == 0.0 and want["mar_100"] == 0.0
    early = dc.image(misses + [gt], scores[:99] + [0.0] * 30 + [scores[99]], [0] * 130, [gt], [0])   # rank 99: kept
    want, _ = _both([early])
    assert want["mar_100"] == 1.0 and want["map"] == pytest.approx(0.01, abs=1e-12)
    rank, matched, _, _, _ = dc.match_all([late])
    assert rank[-1] == 129 and matched[-1] == 0


def test_equal_scores_across_images_keep_insertion_order():
    gt = [0, 0, 100, 100]
    hit = dc.image([gt], [0.5], [0], [gt], [0])
    miss = dc.image([[300, 300, 400, 400]], [0.5], [0], [gt], [0])
    first, _ = _both([hit, miss])
    second, _ = _both([miss, hit])
    assert first["map"] == pytest.approx(51 / 101, abs=1e-12)        # tp, fp: precision 1 up to recall 0.5
    assert second["map"] == pytest.approx(51 * 0.5 / 101, abs=1e-12)  # fp, tp: precision 0.5 up to recall 0.5
    assert first["mar_100"] == second["mar_100"] == 0.5


def test_an_empty_image_and_an_empty_metric():
    from ssl4gie_amd import metrics
    gt = [0, 0, 100, 100]
    case = [dc.image(), dc.image([gt], [0.5], [0], [gt], [0]), dc.image()]
    want, _ = _both(case)
    assert want["map"] == pytest.approx(1.0, abs=1e-12)
    res = metrics.MeanAveragePrecision().compute()
    assert all(float(res[k]) == -1.0 for k in dc.NAMES) and res["classes"].numel() == 0
    m = _metric(case)
    m.reset()
    assert float(m.compute()["map"]) == -1.0


def test_rounding_case_tells_rounded_from_fused_arithmetic():
    """The IoUs of det_map_checks.rounding_case are exactly 0.75 — threshold index 5 — in arithmetic rounded operation
    by operation (numpy, pycocotools' C, the kernel built with contraction off) and 0.75 - 2^-53 with the union as one
    fused multiply-add: the match at index 5 exists in the first and not in the second.  The object must therefore be
    built with contraction off, which the library's -ffp-contract=fast would otherwise override."""
    case = dc.rounding_case()
    assert dc.IOU_THRS[5] == 0.75
    for img in case[:4]:
        d, g = dc.xywh(img["boxes"])[0], dc.xywh(img["gt_boxes"])[0]
        assert dc.iou_matrix(d[None], g[None])[0, 0] == 0.75
        assert dc.fused_iou(d, g) == 0.75 - 2.0 ** -53
        assert dc.evaluate_img(img, 2, 0)["dtm"][:, 0].tolist() == [True] * 6 + [False] * 4
    want, _ = _both(case)
    assert want["map"] == pytest.approx(0.6, abs=1e-12) and want["map_75"] == pytest.approx(1.0, abs=1e-12)
    mk = open(os.path.join(ROOT, "ssl4gie_amd", "csrc", "Makefile")).read()
    assert re.search(r"det_map_ops\.o:\s*CXXFLAGS\s*\+=\s*-ffp-contract=off", mk)


@pytest.mark.parametrize("seed", (1, 2, 3))
def test_torch_path_agrees_with_the_restatement_on_random_cases(seed):
    case = dc.random_case(seed)
    assert dc.margins(case) == 0, "invalid case"
    assert sorted({len(i["scores"]) for i in case}) == sorted(dc.RANDOM_DET_COUNTS)
    assert dc.classes_of(case) == [1, 2, 7] and max(len(i["gt_labels"]) for i in case) == 5
    want, _ = _both(case)
    assert all(want[k] > 0 for k in dc.NAMES), want            # all three area ranges populated and found
    one = _metric(case).compute_f64()
    three = _metric(case, 3).compute_f64()
    assert all(float(one[k]) == float(three[k]) for k in dc.NAMES)


def test_what_is_not_built_is_refused():
    from ssl4gie_amd import metrics
    for kw in ({"box_format": "xywh"}, {"iou_type": "segm"}, {"iou_thresholds": [0.5]}, {"rec_thresholds": [0.0, 1.0]},
               {"max_detection_thresholds": [1, 10, 100]}, {"class_metrics": True}):
        with pytest.raises(NotImplementedError):
            metrics.MeanAveragePrecision(**kw)
    metrics.MeanAveragePrecision(sync_on_compute=False)       # train_detection.py:330
    with pytest.raises(TypeError):
        metrics.MeanAveragePrecision(no_such_option=1)
    preds, target = dc.to_updates(dc.docstring_case())
    for key, val in (("iscrowd", torch.zeros(1, dtype=torch.int64)), ("area", torch.ones(1))):
        with pytest.raises(NotImplementedError):
            metrics.MeanAveragePrecision().update(preds, [{**target[0], key: val}])

    def bad(p, t):
        with pytest.raises(ValueError):
            metrics.MeanAveragePrecision().update(p, t)
    bad(preds, target + target)                                            # lists of different lengths
    bad([{**preds[0], "boxes": preds[0]["boxes"].double()}], target)       # dtypes
    bad([{**preds[0], "scores": preds[0]["scores"].double()}], target)
    bad([{**preds[0], "labels": preds[0]["labels"].int()}], target)
    bad(preds, [{**target[0], "labels": target[0]["labels"].float()}])
    bad([{**preds[0], "boxes": preds[0]["boxes"].reshape(4)}], target)     # shapes
    bad([{**preds[0], "scores": torch.zeros(2)}], target)
    bad([{"boxes": preds[0]["boxes"]}], target)                            # a missing key
    many = 1025
    bad([{"boxes": torch.zeros(many, 4), "scores": torch.zeros(many), "labels": torch.zeros(many, dtype=torch.int64)}],
        target)
    bad(preds, [{"boxes": torch.zeros(many, 4), "labels": torch.zeros(many, dtype=torch.int64)}])
    ok = metrics.MeanAveragePrecision()
    ok.update([{"boxes": torch.zeros(1024, 4), "scores": torch.zeros(1024), "labels": torch.zeros(1024, dtype=torch.int64)}],
              target)
    for label, where in ((256, "pred"), (-1, "pred"), (256, "target")):
        m = metrics.MeanAveragePrecision()
        p, t = dc.to_updates(dc.docstring_case())
        (p if where == "pred" else t)[0]["labels"] = torch.tensor([label])
        m.update(p, t)                                                     # never looks at the values
        with pytest.raises(ValueError):
            m.compute()


def test_header_declares_and_lib_binds_the_det_map_symbols():
    from ssl4gie_amd import _lib
    txt = open(os.path.join(ROOT, "include", "ssl4gie_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    declared = set(re.findall(r"\b(ssl4gie_[a-z0-9_]+)\s*\(", code))
    for name in NEW_SYMBOLS:
        assert name in declared, name
        assert name in _lib.PROTOTYPES, name
    for line in ("train_detection.py:113-151", "eval_detection.py:21-44", "SSL4GIE_DET_MAP_MAX_PER_IMAGE 1024",
                 "SSL4GIE_DET_MAP_CLASSES 256", "SSL4GIE_DET_MAP_CHUNK 256"):
        assert line in txt, line
    assert (_lib.DET_MAP_MAX_PER_IMAGE, _lib.DET_MAP_CLASSES, _lib.DET_MAP_CHUNK) == (1024, 256, 256)
    assert _lib.ABI_VERSION == 13
    L = _lib.load()
    assert L.ssl4gie_abi_version() == 13
    for name in NEW_SYMBOLS:
        assert getattr(L, name) is not None
    srcs = open(os.path.join(ROOT, "ssl4gie_amd", "csrc", "Makefile")).read()
    assert "det_map_ops.hip" in srcs


def test_workspace_queries_and_refused_arguments():
    import ctypes
    from ssl4gie_amd import _lib
    L = _lib.load()
    ws = L.ssl4gie_det_map_workspace_bytes
    assert ws(100, 10000, 200) >= 2 * 10000 * (8 + 4)
    assert ws(5000, 1 << 20, 35000) >= 2 * (1 << 20) * (8 + 4) and ws(1, 2, 1) > 0
    assert ws(1, 1 << 20, 1) > ws(1, 1 << 19, 1)
    for bad in ((0, 10, 10), (-1, 10, 10), (1, 0, 10), (1, -5, 10), (1, 10, 0), (1, 10, -1), (1, (1 << 24) + 1, 1)):
        assert ws(*bad) == 0, bad
    p = 4096  # never dereferenced: every call below is refused before anything is launched
    EARG = 1000
    thr = (ctypes.c_double * 10)(*dc.IOU_THRS)
    rec = (ctypes.c_double * 101)(*dc.REC_THRS)
    match = lambda **kw: L.ssl4gie_det_map_match(*[kw.get(k, v) for k, v in (
        ("db", p), ("ds", p), ("dl", p), ("do", p), ("gb", p), ("gl", p), ("go", p), ("n_img", 2), ("n_det", 8), ("n_gt", 4),
        ("thr", thr), ("rank", p), ("matched", p), ("ignored", p), ("npig", p), ("present", p), ("flag", p), ("st", None))])
    for kw in ({"db": None}, {"ds": None}, {"dl": None}, {"do": None}, {"gb": None}, {"gl": None}, {"go": None},
               {"thr": None}, {"rank": None}, {"matched": None}, {"ignored": None}, {"npig": None}, {"present": None},
               {"flag": None}, {"n_img": 0}, {"n_img": -1}, {"n_det": -1}, {"n_gt": -1}, {"n_det": (1 << 24) + 1}):
        assert match(**kw) == EARG, kw
    order = lambda **kw: L.ssl4gie_det_map_order(*[kw.get(k, v) for k, v in (
        ("ds", p), ("dl", p), ("rank", p), ("n", 8), ("idx", p), ("seg", p), ("ws", p), ("st", None))])
    for kw in ({"ds": None}, {"dl": None}, {"rank": None}, {"idx": None}, {"seg": None}, {"ws": None}, {"n": 0},
               {"n": -3}, {"n": (1 << 24) + 1}, {"ws": p + 4}):
        assert order(**kw) == EARG, kw
    acc = lambda **kw: L.ssl4gie_det_map_accumulate(*[kw.get(k, v) for k, v in (
        ("idx", p), ("seg", p), ("rank", p), ("matched", p), ("ignored", p), ("npig", p), ("present", p), ("flag", p),
        ("n", 8), ("rec", rec), ("stats", p), ("o64", p), ("o32", p), ("oi", p), ("st", None))])
    for kw in ({"idx": None}, {"seg": None}, {"rank": None}, {"matched": None}, {"ignored": None}, {"npig": None},
               {"present": None}, {"flag": None}, {"rec": None}, {"stats": None}, {"o64": None}, {"o32": None},
               {"oi": None}, {"n": -1}, {"n": (1 << 24) + 1}):
        assert acc(**kw) == EARG, kw
