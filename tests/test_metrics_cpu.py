"""CPU: the torch formulations of ssl4gie_amd.metrics reproduce the reference's own results (tests/golden/
g20_metrics.npz, written by make_golden_metrics.py from the reference's classes and functions), the accumulators agree
with the per-call classes, tests/metric_checks.py's fp64 restatements agree with both, and the C ABI declares, binds and
exports the metric entry points — with the arguments they refuse before any launch."""
import math
import os
import re

import numpy as np
import pytest
import torch

import metric_checks as mc
from conftest import ROOT, load_golden

NEW_SYMBOLS = ("ssl4gie_seg_counts", "ssl4gie_seg_scores", "ssl4gie_confusion_update", "ssl4gie_confusion_scores",
               "ssl4gie_lower_median_workspace_bytes", "ssl4gie_lower_median_f32", "ssl4gie_depth_eval_workspace_bytes",
               "ssl4gie_depth_eval")
SEG_KEYS = ("0", "1", "2", "3")


def close(a, b, rel=1e-6):
    return abs(float(a) - float(b)) <= rel * abs(float(b))


@pytest.fixture(scope="module")
def g20():
    return load_golden("g20_metrics.npz")


def test_segmentation_classes_reproduce_the_reference_fixture(g20):
    from ssl4gie_amd import metrics
    fns = (metrics.DiceScore(), metrics.IoU(), metrics.Precision(), metrics.Recall())
    for k in SEG_KEYS:
        logits, target = torch.from_numpy(g20[f"seg/{k}/logits"]), torch.from_numpy(g20[f"seg/{k}/target"])
        for f, want in zip(fns, g20[f"seg/{k}/scores"]):
            got = f(logits, target)
            assert got.dim() == 0 and got.device == logits.device
            assert close(got, want), (k, type(f).__name__, float(got), float(want))
    logits, target = torch.from_numpy(g20["seg/nosig/logits"]), torch.from_numpy(g20["seg/nosig/target"])
    for f, want in zip(fns, g20["seg/nosig/scores"]):
        assert close(f(logits, target, sigmoid=False), want)
    assert g20["seg/3/scores"].tolist() == [2.0, 1.0, 1.0, 1.0]   # empty prediction on an empty target
    assert float(metrics.DiceScore()(torch.from_numpy(g20["seg/3/logits"]), torch.from_numpy(g20["seg/3/target"]))) == 2.0


def test_segmentation_accumulator_on_cpu_is_the_mean_over_images(g20):
    from ssl4gie_amd import metrics
    acc = metrics.SegmentationScores()
    per_image = []
    for k in SEG_KEYS:
        logits, target = torch.from_numpy(g20[f"seg/{k}/logits"]), torch.from_numpy(g20[f"seg/{k}/target"])
        mean = acc.update(logits, target)
        assert np.allclose(mean.numpy(), g20[f"seg/{k}/scores"], rtol=1e-6, atol=0)
        counts, _ = mc.seg_counts64(logits[:, 0], target[:, 0])
        per_image.append(mc.seg_scores32(counts, 1e-8).double())
    want = torch.cat(per_image, 1).mean(1)
    got = acc.compute()
    for i, name in enumerate(acc.names):
        assert close(got[name], want[i], 1e-12), (name, got[name], float(want[i]))
    # the logits at another size than the target: resampled to the target's
    g = torch.Generator().manual_seed(3)
    logits, target = 3 * torch.randn(2, 1, 16, 16, generator=g), (torch.rand(2, 1, 23, 29, generator=g) < 0.4).float()
    acc2 = metrics.SegmentationScores()
    mean = acc2.update(logits, target, size=(23, 29))
    counts, _ = mc.seg_counts64(logits[:, 0], target[:, 0])
    assert np.allclose(mean.numpy(), mc.seg_scores32(counts, 1e-8).mean(1).numpy(), rtol=1e-6, atol=0)
    with pytest.raises(ValueError):
        acc2.update(logits, target, size=(16, 16))


def test_classification_classes_and_accumulator_reproduce_the_reference_fixture(g20):
    from ssl4gie_amd import metrics
    for C in (6, 23):
        preds, targets = torch.from_numpy(g20[f"cls/{C}/preds"]), torch.from_numpy(g20[f"cls/{C}/targets"])
        want = g20[f"cls/{C}/scores"]
        absent = [c for c in range(C) if not ((preds == c).any() or (targets == c).any())]
        assert absent, "the fixture must hold a class absent from predictions and targets"
        for f, w in zip((metrics.meanF1Score(C), metrics.meanPrecision(C), metrics.meanRecall(C)), want):
            got = f(preds, targets)
            assert got.dim() == 0 and close(got, w), (C, type(f).__name__, float(got), float(w))
        assert np.allclose(mc.class_loop32(preds, targets, C, 1e-8).numpy(), want, rtol=1e-6, atol=0)
        acc = metrics.ClassificationScores(C)
        for chunk_p, chunk_t in zip(preds.split(17), targets.split(17)):
            acc.update(chunk_p, chunk_t)
        conf, rejected = mc.confusion64(preds, targets, C)
        assert torch.equal(acc.matrix, conf) and rejected == 0
        res = acc.compute()
        assert close(res["f1"], want[0]) and close(res["precision"], want[1]) and close(res["recall"], want[2])
        assert close(res["accuracy"], float((preds == targets).float().mean())) and res["rejected"] == 0
        terms = mc.class_terms32(conf, 1e-8)
        assert all(float(terms[0, c]) == 2.0 and float(terms[1, c]) == 1.0 and float(terms[2, c]) == 1.0 for c in absent)
    # logits instead of predictions, and labels outside [0, C)
    logits, targets = mc.class_case(64, 6, seed=5)
    targets[3], targets[9] = -1, 6
    acc = metrics.ClassificationScores(6)
    acc.update(logits, targets)
    conf, rejected = mc.confusion64(torch.argmax(logits, 1), targets, 6)
    assert torch.equal(acc.matrix, conf) and acc.compute()["rejected"] == rejected == 2


def test_depth_functions_reproduce_the_reference_fixture(g20):
    from ssl4gie_amd import metrics
    scale_ = float(g20["depth/scale_"])
    acc = metrics.DepthErrors(scale=scale_)
    rows = []
    for k in range(3):
        pred, target = torch.from_numpy(g20[f"depth/{k}/pred"]), torch.from_numpy(g20[f"depth/{k}/target"])
        target_og = torch.from_numpy(g20[f"depth/{k}/target_og"])
        keep = target_og.clone()
        got = acc.update(pred, target, target_og)
        assert torch.equal(target_og, keep), "target_og must not be modified"
        want = g20[f"depth/{k}/errors"]
        assert got.shape == (1, 3) and np.allclose(got[0].numpy(), want, rtol=1e-6, atol=0), (k, got, want)
        f64 = mc.depth_errors64(pred, target, target_og[:, 0], scale_)
        assert float(mc.rel_dev(torch.from_numpy(want)[None], f64).max()) < 1e-4   # the restatement describes the same thing
        rows.append(want.astype(np.float64))
    res = acc.compute()
    for i, name in enumerate(acc.names):
        assert close(res[name], np.mean([r[i] for r in rows]), 1e-7)
    # the three functions themselves: the reference's arguments, a 0-dim tensor instead of a float
    g = torch.Generator().manual_seed(9)
    p, t = torch.rand(5, 7, generator=g), torch.rand(5, 7, generator=g)
    t[t < 0.3] = 0
    v = t > 0
    assert float(metrics.rmse(p, t)) == float(torch.sqrt(torch.mean((p - t)[v] ** 2)))
    assert float(metrics.rel_err(p, t)) == float(torch.median(torch.abs((p - t) / t)[v]))
    assert float(metrics.abs_err(p, t)) == float(torch.mean(torch.abs(p - t)[v]))
    assert metrics.rmse(p, t).dim() == 0
    assert math.isnan(float(metrics.rel_err(p, torch.zeros_like(t))))


def test_lower_median_on_cpu_is_torch_median():
    from ssl4gie_amd import metrics
    for kind in mc.MEDIAN_KINDS:
        for n in mc.MEDIAN_NS[:7]:
            x = mc.median_case(kind, n)
            assert float(metrics.lower_median(x)) == float(torch.sort(x).values[(n - 1) // 2]), (kind, n)
    assert math.isnan(float(metrics.lower_median(torch.empty(0))))


def test_crop_offset_rounds_half_to_even():
    from ssl4gie_amd import metrics
    assert [metrics.crop_offset(29, h) for h in (29, 28, 24, 23, 22, 16)] == [0, 0, 2, 3, 4, 6]   # 0.5 -> 0, 2.5 -> 2, 3.5 -> 4
    assert [mc.crop_offset(29, h) for h in (28, 24, 22)] == [0, 2, 4]


def test_depth_gate_inputs_are_sane():
    """the special images of the GPU test's cases do what they are there for, in the reference's fp32 formulation"""
    from ssl4gie_amd import metrics
    pred, target, og = mc.depth_case(16, 23, 29, seed=1)
    ref = metrics.depth_errors_torch(pred, target, og, mc.SCALE_)
    f64 = mc.depth_errors64(pred, target, og, mc.SCALE_)
    assert torch.isnan(ref[2]).all() and torch.isnan(f64[2]).all()           # no valid pixel
    assert not torch.isnan(ref[[0, 1, 3]]).any()
    # a constant prediction: det == 0, scale = shift = 0, the prediction is 0 everywhere: |d / t| == 1
    assert float(ref[3, 1]) == 1.0 and float(f64[3, 1]) == 1.0
    assert float(mc.rel_dev(ref, f64).max()) < 1e-3


def test_header_declares_and_lib_binds_the_metric_symbols():
    from ssl4gie_amd import _lib
    txt = open(os.path.join(ROOT, "include", "ssl4gie_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    declared = set(re.findall(r"\b(ssl4gie_[a-z0-9_]+)\s*\(", code))
    for name in NEW_SYMBOLS:
        assert name in declared, name
        assert name in _lib.PROTOTYPES, name
    assert "SSL4GIE_PRED_I64 2" in txt and _lib.PRED_I64 == 2
    assert _lib.ABI_VERSION == 13
    L = _lib.load()   # resolves every bound symbol in the built library
    assert L.ssl4gie_abi_version() == 13
    for name in NEW_SYMBOLS:
        assert getattr(L, name) is not None
    srcs = open(os.path.join(ROOT, "ssl4gie_amd", "csrc", "Makefile")).read()
    assert "metric_ops.hip" in srcs


def test_workspace_queries_and_refused_arguments():
    from ssl4gie_amd import _lib
    L = _lib.load()
    assert L.ssl4gie_lower_median_workspace_bytes() >= 2048 * 8
    big = L.ssl4gie_depth_eval_workspace_bytes(1, 224, 1080, 1350)
    assert big >= 4 * 1080 * 1350 and big % 4 == 0
    assert L.ssl4gie_depth_eval_workspace_bytes(3, 16, 23, 29) > L.ssl4gie_depth_eval_workspace_bytes(2, 16, 23, 29)
    for bad in ((0, 16, 8, 8), (1, 0, 8, 8), (1, 16, 0, 8), (1, 16, 8, -1)):
        assert L.ssl4gie_depth_eval_workspace_bytes(*bad) == 0
    p = 4096  # never dereferenced: every call below is refused before anything is launched
    EARG = 1000
    assert L.ssl4gie_depth_eval(p, p, p, p, 1, 16, 17, 8, 8, 10.0, p, None) == EARG          # not square
    assert L.ssl4gie_depth_eval(p, p, p, p, 1, 0, 0, 8, 8, 10.0, p, None) == EARG
    assert L.ssl4gie_depth_eval(p, p, p, p, 1, 16, 16, 0, 8, 10.0, p, None) == EARG
    assert L.ssl4gie_depth_eval(p, p, p, p, 1, 16, 16, 8, -3, 10.0, p, None) == EARG
    assert L.ssl4gie_depth_eval(p, p, None, p, 1, 16, 16, 8, 8, 10.0, p, None) == EARG
    assert L.ssl4gie_seg_counts(p, 0, p, 1, p, 1, 8, 8, 8, 8, 1, None) == EARG               # target dtype u16
    assert L.ssl4gie_seg_counts(p, 7, p, 0, p, 1, 8, 8, 8, 8, 1, None) == EARG
    assert L.ssl4gie_seg_counts(p, 0, p, 0, p, 0, 8, 8, 8, 8, 1, None) == EARG
    assert L.ssl4gie_seg_counts(p, 0, p, 0, p, 1, 8, 8, 65536, 65536, 1, None) == EARG
    assert L.ssl4gie_seg_scores(p, 0, 1e-8, p, None, None) == EARG
    assert L.ssl4gie_confusion_update(p, 3, p, p, p, 4, 6, None) == EARG
    assert L.ssl4gie_confusion_update(p, 0, p, p, None, 4, 6, None) == EARG
    assert L.ssl4gie_confusion_update(p, 0, p, p, p, 4, 0, None) == EARG
    assert L.ssl4gie_confusion_scores(p, 0, 1e-8, p, None) == EARG
    assert L.ssl4gie_lower_median_f32(p, -1, p, p, None) == EARG
    assert L.ssl4gie_lower_median_f32(None, 4, p, p, None) == EARG
