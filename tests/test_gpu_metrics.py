"""GPU: the evaluation-metric kernels (csrc/metric_ops.hip) and ssl4gie_amd.metrics on the device against the fp64
restatements of tests/metric_checks.py and the reference's own results (tests/golden/g20_metrics.npz).

Gates.  Counts and the confusion matrix are integers: equality.  A score from counts is one correctly rounded fp32
division and at most three additions: 2 ulp.  The counts of a resampled map may differ from the fp64 restatement's by
the number of pixels whose fp64 value lies within 1e-4 of the threshold.  The median is a select: bit equality.  The
depth errors depend on the conditioning of the 2 x 2 solve, so their gate is measured, per output, as 4 x the largest
error over this file's cases of the REFERENCE's fp32 formulation on the CPU against the fp64 restatement — never
against the device path itself."""
import math

import numpy as np
import pytest
import torch

import metric_checks as mc
from conftest import load_golden

pytestmark = pytest.mark.gpu
DEV = "cuda"
SMOOTH = 1e-8


def _ops():
    from ssl4gie_amd import ops
    return ops


# ------------------------------------------------------------------ segmentation
@pytest.mark.parametrize("ldt", (torch.float32, torch.bfloat16), ids=("f32", "bf16"))
@pytest.mark.parametrize("tdt", (torch.float32, torch.uint8), ids=("tgt_f32", "tgt_u8"))
def test_seg_counts_without_resize_are_exact(ldt, tdt):
    ops = _ops()
    for B in (1, 3):
        for H, W in ((7, 5), (16, 16), (33, 40), (224, 224)):
            logits, target = mc.seg_case(B, H, W, seed=100 * B + H)
            logits = logits.to(ldt)
            assert float(logits.float().abs().min()) >= 9e-4
            want, _ = mc.seg_counts64(logits, target)
            got = ops.seg_counts(logits.to(DEV), target.to(tdt).to(DEV), True)
            assert got.dtype == torch.int64 and torch.equal(got.cpu(), want), (B, H, W, got.cpu(), want)
            if B == 3:
                assert want[0].tolist() == [0, 0, 0] and int(want[1, 0]) == H * W      # empty / empty, all-positive
                dice = ops.seg_scores(got[0:1].contiguous(), SMOOTH)
                assert dice.cpu().tolist() == [2.0, 1.0, 1.0, 1.0]
    # sigmoid=False thresholds the value itself at 0.5; an odd pointer offset takes the scalar path
    g = torch.Generator().manual_seed(5)
    probs, target = torch.rand(2, 16, 16, generator=g), (torch.rand(2, 16, 16, generator=g) < 0.5).float()
    assert torch.equal(ops.seg_counts(probs.to(ldt).to(DEV), target.to(tdt).to(DEV), False).cpu(),
                       mc.seg_counts64(probs.to(ldt), target, sigmoid=False)[0])
    buf_l = torch.zeros(2 * 256 + 1, dtype=ldt, device=DEV)
    buf_t = torch.zeros(2 * 256 + 1, dtype=tdt, device=DEV)
    buf_l[1:] = probs.to(ldt).reshape(-1).to(DEV)
    buf_t[1:] = target.to(tdt).reshape(-1).to(DEV)
    got = ops.seg_counts(buf_l[1:].view(2, 16, 16), buf_t[1:].view(2, 16, 16), False)
    assert torch.equal(got.cpu(), mc.seg_counts64(probs.to(ldt), target, sigmoid=False)[0])


@pytest.mark.parametrize("sin,hw", ((16, (23, 29)), (224, (301, 257)), (64, (40, 33))), ids=("16to23x29", "224to301x257", "64to40x33"))
@pytest.mark.parametrize("ldt", (torch.float32, torch.bfloat16), ids=("f32", "bf16"))
def test_seg_counts_with_resize(sin, hw, ldt):
    ops = _ops()
    g = torch.Generator().manual_seed(sin)
    B = 2
    logits = (3.0 * torch.randn(B, sin, sin, generator=g)).to(ldt)
    target = (torch.rand(B, *hw, generator=g) < 0.4).float()
    want, v64 = mc.seg_counts64(logits, target)
    band = (v64.abs() < 1e-4).reshape(B, -1).sum(1)
    assert int(band.max()) <= 1e-3 * hw[0] * hw[1], "invalid case: too many pixels at the threshold"
    got = ops.seg_counts(logits.to(DEV), target.to(DEV), True).cpu()
    diff = (got - want).abs()
    print(f"resize {sin}^2 -> {hw}: band pixels {band.tolist()}, count differences {diff.tolist()}")
    assert torch.equal(got[:, 1], want[:, 1])
    assert bool((diff <= band.view(B, 1)).all()), (got, want, band)


def test_seg_scores_from_counts_and_accumulator():
    ops = _ops()
    counts = torch.tensor([[0, 0, 0], [10, 0, 0], [0, 7, 0], [5, 5, 5], [17, 23, 11], [50176, 20000, 19999],
                           [1458000, 700001, 333333], [3, 1, 1], [2 ** 26 + 1, 2 ** 25 + 3, 2 ** 25 + 1]], dtype=torch.int64)
    ref = mc.seg_scores32(counts, SMOOTH)                                   # [4, n], the reference's fp32 formulas
    for i in range(counts.shape[0]):
        got = ops.seg_scores(counts[i:i + 1].to(DEV), SMOOTH).cpu()
        for k in range(4):
            assert abs(float(got[k]) - float(ref[k, i])) <= 2 * mc.ulp32(ref[k, i]), (i, k, float(got[k]), float(ref[k, i]))
    got = ops.seg_scores(counts.to(DEV), SMOOTH).cpu()
    mean = ref.double().mean(1)
    for k in range(4):
        assert abs(float(got[k]) - float(mean[k])) <= 2 * mc.ulp32(mean[k])
    # three updates of one image each: the accumulator holds the sum of the three calls' scores, and the image count
    from ssl4gie_amd import metrics
    acc = metrics.SegmentationScores(SMOOTH)
    calls = []
    for seed in (1, 2, 3):
        logits, target = mc.seg_case(1, 33, 40, seed=seed)
        calls.append(acc.update(logits.view(1, 1, 33, 40).to(DEV), target.view(1, 1, 33, 40).to(DEV)).cpu().double())
    assert acc.accum.dtype == torch.float64 and acc.accum.is_cuda
    assert torch.equal(acc.accum[:4].cpu(), calls[0] + calls[1] + calls[2]) and float(acc.accum[4]) == 3.0
    res = acc.compute()
    assert res["dice"] == float((calls[0] + calls[1] + calls[2])[0] / 3.0)
    # batches of several images: sum over images of the per-image scores
    acc = metrics.SegmentationScores(SMOOTH)
    total = torch.zeros(4, dtype=torch.float64)
    for B, seed in ((2, 4), (3, 5), (1, 6)):
        logits, target = mc.seg_case(B, 16, 16, seed=seed)
        acc.update(logits.unsqueeze(1).to(DEV), target.unsqueeze(1).to(DEV))
        total += mc.seg_scores32(mc.seg_counts64(logits, target)[0], SMOOTH).double().sum(1)
    assert torch.allclose(acc.accum[:4].cpu(), total, rtol=1e-7, atol=0) and float(acc.accum[4]) == 6.0


# ------------------------------------------------------------------ classification
@pytest.mark.parametrize("C", (2, 6, 23))
def test_confusion_matrix_is_exact(C):
    ops = _ops()
    for B in (1, 5, 257):
        for dt in (torch.float32, torch.bfloat16):
            logits, targets = mc.class_case(B, C, seed=C * 1000 + B, dtype=dt)
            preds = torch.argmax(logits.float(), 1)                      # the CPU's argmax: the first maximum
            if B == 257:
                assert (logits.float() == logits.float().max(1, keepdim=True).values).sum(1).max() > 1, "no tie in the case"
            want, _ = mc.confusion64(preds, targets, C)
            conf = torch.zeros(C * C + 1, dtype=torch.int64, device=DEV)
            ops.confusion_update(conf, logits.to(DEV), targets.to(DEV))
            assert torch.equal(conf[:-1].view(C, C).cpu(), want) and int(conf[-1]) == 0, (B, dt)
            if C > 2:
                assert int(want[C - 1].sum()) == 0                       # a class that never occurs as a target
            # predictions instead of logits, with labels outside [0, C): rejected, the matrix is left alone
            bad_t, bad_p = targets.clone(), preds.clone()
            bad_t[0] = C
            if B >= 5:
                bad_t[1], bad_p[2] = -1, C + 3
            want2, rejected = mc.confusion64(bad_p, bad_t, C)
            conf2 = torch.zeros(C * C + 1, dtype=torch.int64, device=DEV)
            ops.confusion_update(conf2, bad_p.to(DEV), bad_t.to(DEV))
            assert torch.equal(conf2[:-1].view(C, C).cpu(), want2) and int(conf2[-1]) == rejected == (3 if B >= 5 else 1)
            only_bad = torch.zeros(C * C + 1, dtype=torch.int64, device=DEV)
            ops.confusion_update(only_bad, logits[:1].to(DEV), torch.tensor([C], device=DEV))
            assert int(only_bad[:-1].abs().sum()) == 0 and int(only_bad[-1]) == 1


def test_confusion_scores_and_accumulation():
    ops = _ops()
    from ssl4gie_amd import metrics
    g20 = load_golden("g20_metrics.npz")
    for C in (6, 23):
        preds, targets = torch.from_numpy(g20[f"cls/{C}/preds"]), torch.from_numpy(g20[f"cls/{C}/targets"])
        conf = torch.zeros(C * C + 1, dtype=torch.int64, device=DEV)
        ops.confusion_update(conf, preds.to(DEV), targets.to(DEV))
        got = ops.confusion_scores(conf, SMOOTH).cpu()
        want64, _ = mc.confusion64(preds, targets, C)
        terms = mc.class_terms32(want64, SMOOTH)                          # [3, C] fp32
        loop = mc.class_loop32(preds, targets, C, SMOOTH)
        for k in range(3):
            tol = 2 * sum(mc.ulp32(t) for t in terms[k]) / C              # 2 ulp per class term
            assert abs(float(got[k]) - float(terms[k].double().mean())) <= tol, (C, k)
            assert abs(float(got[k]) - float(loop[k])) <= tol, (C, k, float(got[k]), float(loop[k]))
            assert abs(float(got[k]) - float(g20[f"cls/{C}/scores"][k])) <= tol, (C, k)
        acc_want = float((preds == targets).sum()) / len(preds)
        assert abs(float(got[3]) - acc_want) <= mc.ulp32(acc_want)
    # more classes than the kernel forms terms for at a time: still the loop's order
    C = 1030
    g = torch.Generator().manual_seed(12)
    targets = torch.randint(0, C - 5, (4096,), generator=g)
    preds = torch.where(torch.rand(4096, generator=g) < 0.5, targets, torch.randint(0, C, (4096,), generator=g))
    conf = torch.zeros(C * C + 1, dtype=torch.int64, device=DEV)
    ops.confusion_update(conf, preds.to(DEV), targets.to(DEV))
    want64, _ = mc.confusion64(preds, targets, C)
    assert torch.equal(conf[:-1].view(C, C).cpu(), want64)
    got = ops.confusion_scores(conf, SMOOTH).cpu()
    terms = mc.class_terms32(want64, SMOOTH).numpy()
    for k in range(3):
        seq = np.add.accumulate(terms[k], dtype=np.float32)[-1] / np.float32(C)
        assert abs(float(got[k]) - float(seq)) <= 2 * sum(mc.ulp32(t) for t in terms[k]) / C, (k, float(got[k]), float(seq))
    # seven batches accumulate to one pass over their concatenation
    C = 23
    batches = [mc.class_case(B, C, seed=70 + i) for i, B in enumerate((64, 64, 1, 5, 257, 64, 33))]
    acc = metrics.ClassificationScores(C)
    for logits, targets in batches:
        acc.update(logits.to(DEV), targets.to(DEV))
    one = metrics.ClassificationScores(C)
    one.update(torch.cat([b[0] for b in batches]).to(DEV), torch.cat([b[1] for b in batches]).to(DEV))
    assert torch.equal(acc.conf, one.conf) and torch.equal(acc.scores(), one.scores())
    want, _ = mc.confusion64(torch.argmax(torch.cat([b[0] for b in batches]), 1), torch.cat([b[1] for b in batches]), C)
    assert torch.equal(acc.matrix.cpu(), want)


# ------------------------------------------------------------------ median
@pytest.mark.parametrize("kind", mc.MEDIAN_KINDS)
def test_lower_median_is_torch_median_bit_for_bit(kind):
    ops = _ops()
    for n in mc.MEDIAN_NS:
        x = mc.median_case(kind, n)
        xd = x.to(DEV)
        got = ops.lower_median(xd)
        want = torch.median(x)
        assert got.dim() == 0 and got.dtype == torch.float32
        assert got.cpu().view(torch.int32).item() == want.view(torch.int32).item(), (kind, n, float(got), float(want))
        assert torch.equal(xd.cpu(), x), "the input must not be modified"
        assert torch.equal(ops.lower_median(xd), got)                   # run to run
    if kind == "random":
        assert math.isnan(float(ops.lower_median(torch.empty(0, device=DEV))))
        buf = mc.median_case("random", 1001).to(DEV)                    # a base that is not 16-byte aligned
        assert float(ops.lower_median(buf[1:])) == float(torch.median(buf[1:].cpu()))


# ------------------------------------------------------------------ depth
@pytest.fixture(scope="module")
def depth_cases():
    """per shape: inputs, the fp64 restatement and the reference's fp32 formulation on the CPU; and the gate per
    output = 4 x the largest relative error of the latter against the former over ALL cases (the fixture's included)"""
    from ssl4gie_amd import metrics
    cases = []
    for i, (S, H, W) in enumerate(mc.DEPTH_SHAPES):
        pred, target, og = mc.depth_case(S, H, W, seed=40 + i)
        cases.append(dict(name=f"S{S}_{H}x{W}", pred=pred, target=target, og=og, scale=mc.SCALE_))
    g20 = load_golden("g20_metrics.npz")
    for k in range(3):
        cases.append(dict(name=f"g20_{k}", pred=torch.from_numpy(g20[f"depth/{k}/pred"]),
                          target=torch.from_numpy(g20[f"depth/{k}/target"]),
                          og=torch.from_numpy(g20[f"depth/{k}/target_og"])[:, 0].contiguous(),
                          scale=float(g20["depth/scale_"]), recorded=torch.from_numpy(g20[f"depth/{k}/errors"])))
    worst = torch.zeros(3, dtype=torch.float64)
    for c in cases:
        c["f64"] = mc.depth_errors64(c["pred"], c["target"], c["og"], c["scale"])
        c["ref32"] = metrics.depth_errors_torch(c["pred"], c["target"], c["og"], c["scale"])
        if "recorded" in c:
            assert torch.allclose(c["ref32"][0], c["recorded"], rtol=1e-6, atol=0), "the CPU formulation is the reference's"
        c["ref_err"] = mc.rel_dev(c["ref32"], c["f64"])
        worst = torch.maximum(worst, c["ref_err"].max(0).values)
    assert bool((worst > 0).all()) and bool((worst < 1e-3).all()), worst
    return cases, 4.0 * worst


def test_depth_eval_against_fp64(depth_cases):
    ops = _ops()
    cases, gate = depth_cases
    print(f"depth gates (4 x the reference's worst fp32 error): rmse {gate[0]:.3e} rel_err {gate[1]:.3e} abs_err {gate[2]:.3e}")
    for c in cases:
        og_dev = c["og"].to(DEV)
        got = ops.depth_eval(c["pred"].to(DEV), c["target"].to(DEV), og_dev, c["scale"])
        assert torch.equal(og_dev.cpu(), c["og"]), "target_og must not be modified"
        err = mc.rel_dev(got.cpu(), c["f64"])
        print(f"{c['name']}: device error {err.max(0).values.tolist()}, reference fp32 error {c['ref_err'].max(0).values.tolist()}")
        assert bool((err <= gate).all()), (c["name"], err, gate)
        again = ops.depth_eval(c["pred"].to(DEV), c["target"].to(DEV), og_dev, c["scale"])
        assert torch.equal(again.view(torch.int32), got.view(torch.int32))   # run to run, the NaNs included
        if c["pred"].shape[0] == 4:
            assert torch.isnan(got[2]).all() and float(got[3, 1]) == 1.0   # no valid pixel; det == 0: |0 - t| / t


def test_depth_eval_median_is_the_median_of_its_own_array():
    """scale = 1, shift = 0 (pred == target on the valid pixels) and an identity resize: the aligned prediction is pred
    itself, so |d / t| can be recomputed in torch on the device and its median must come out bit for bit"""
    ops = _ops()
    g = torch.Generator().manual_seed(77)
    for S in (16, 61):
        pred = (0.1 + 0.8 * torch.rand(2, S, S, generator=g)).to(DEV)
        target = pred.clone()
        target[torch.rand(2, S, S, generator=g).to(DEV) < 0.25] = 0
        og = torch.rand(2, S, S, generator=g)
        og[torch.rand(2, S, S, generator=g) < 0.25] = 0
        og = og.to(DEV)
        got = ops.depth_eval(pred, target, og, mc.SCALE_)
        o = pred.clamp(0.0, 1.0) * mc.SCALE_
        t = og * mc.SCALE_
        for b in range(2):
            v = t[b] > 0
            rel = ((o[b] - t[b]) / t[b]).abs()[v]
            assert got[b, 1].view(torch.int32).item() == torch.median(rel).view(torch.int32).item(), (S, b)
            assert float(got[b, 1]) == float(torch.median(rel.cpu()))


# ------------------------------------------------------------------ modules
def test_reference_named_classes_agree_with_the_accumulators(depth_cases, monkeypatch):
    from ssl4gie_amd import metrics
    cases, gate = depth_cases
    logits, target = mc.seg_case(3, 33, 40, seed=9)
    logits, target = logits.unsqueeze(1).to(DEV), target.unsqueeze(1).to(DEV)
    seg_fns = (metrics.DiceScore(), metrics.IoU(), metrics.Precision(), metrics.Recall())
    cls_logits, cls_targets = mc.class_case(257, 23, seed=11)
    preds = torch.argmax(cls_logits, 1).to(DEV)
    cls_fns = (metrics.meanF1Score(23), metrics.meanPrecision(23), metrics.meanRecall(23))
    c = cases[0]
    x = mc.median_case("random", 257).to(DEV)

    def run():
        acc = metrics.SegmentationScores()
        batch = acc.update(logits, target)
        seg = torch.stack([f(logits, target) for f in seg_fns])
        assert seg.is_cuda and seg[0].dim() == 0
        assert torch.equal(seg, batch) and [float(v) for v in seg.cpu()] == pytest.approx(list(acc.compute().values()), rel=1e-6)
        cacc = metrics.ClassificationScores(23)
        cacc.update(preds, cls_targets.to(DEV))
        cls = torch.stack([f(preds, cls_targets.to(DEV)) for f in cls_fns])
        assert cls.is_cuda and torch.allclose(cls, cacc.scores()[:3], rtol=1e-6, atol=0)
        dacc = metrics.DepthErrors(scale=c["scale"])
        d = dacc.update(c["pred"].unsqueeze(1).to(DEV), c["target"].unsqueeze(1).to(DEV), c["og"].unsqueeze(1).to(DEV))
        med = metrics.lower_median(x)
        return seg.cpu(), cls.cpu(), d.cpu(), med.cpu()

    fused = run()
    monkeypatch.setenv("SSL4GIE_FUSED_METRICS", "0")
    torch_path = run()
    assert torch.allclose(fused[0], torch_path[0], rtol=4 * mc.EPS32, atol=0)   # exact counts, fp32 formulas, another batch sum
    assert torch.allclose(fused[1], torch_path[1], rtol=4 * mc.EPS32, atol=0)
    assert bool((mc.rel_dev(fused[2], c["f64"]) <= gate).all()) and bool((mc.rel_dev(torch_path[2], c["f64"]) <= gate).all())
    assert torch.equal(fused[3], torch_path[3])
    # the depth functions on device tensors: 0-dim device tensors, rel_err through the select
    p, t = c["pred"][0].to(DEV), c["target"][0].to(DEV)
    monkeypatch.delenv("SSL4GIE_FUSED_METRICS")
    vals = [f(p, t) for f in (metrics.rmse, metrics.rel_err, metrics.abs_err)]
    assert all(v.is_cuda and v.dim() == 0 for v in vals)
    v = t.cpu() > 0
    assert float(vals[1]) == float(torch.median(((p.cpu() - t.cpu()) / t.cpu()).abs()[v]))
