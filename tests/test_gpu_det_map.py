"""GPU: the detection-metric kernels (csrc/det_map_ops.hip) and ssl4gie_amd.metrics.MeanAveragePrecision on the device
against the fp64 restatement of tests/det_map_checks.py.

Gates.  Ranks, the two 40-bit masks, npig, the sorted order and the class segments are integers: equality.  Every
decision behind them is an fp64 operation rounded as numpy rounds it, and the random cases keep 1e-9 (IoU) / 1e-3 px^2
(area) away from every bound (`margins(case) == 0`), so a difference is never a rounding tie.  The case `rounding`
is the opposite: IoUs that equal the threshold 0.75 exactly when each fp64 operation is rounded on its own and miss it
by one ulp when the union is contracted into a fused multiply-add (det_map_checks.rounding_case) — equality there
shows that the library was built with contraction off.  The summaries add at most
1010 K terms in [0, 1] in another order than numpy's pairwise mean: <= 3e-11, gate 1e-9."""
import functools

import numpy as np
import pytest
import torch

import det_map_checks as dc

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _ops():
    from ssl4gie_amd import ops
    return ops


@functools.lru_cache(maxsize=None)
def _case(name):
    if name.startswith("random"):
        case = dc.random_case(int(name[6:]))
        assert dc.margins(case) == 0, "invalid case"
        return case
    return {"shape3": lambda: dc.shape_case((1, 2, 7)), "shape1": lambda: dc.shape_case((4,), seed=12),
            "exact": dc.exact_case, "rounding": dc.rounding_case, "segments": dc.segment_case, "docstring": dc.docstring_case}[name]()


@functools.lru_cache(maxsize=None)
def _match_ref(name):
    return dc.match_all(_case(name))


@functools.lru_cache(maxsize=None)
def _restated(name):
    precision, recall, classes = dc.accumulate(_case(name))
    return precision, recall, classes, dc.summarize(precision, recall)


def _match(case):
    return _ops().det_map_match(*dc.flat(case, DEV))


@pytest.mark.parametrize("name", ("random1", "random2", "shape3", "shape1", "exact", "rounding", "segments"))
def test_match_rank_masks_and_npig_equal_the_restatement(name):
    case = _case(name)
    rank, matched, ignored, npig, present, flag = _match(case)
    w_rank, w_matched, w_ignored, w_npig, w_present = _match_ref(name)
    assert int(flag.cpu()) == 0
    assert np.array_equal(rank.cpu().numpy(), w_rank), np.nonzero(rank.cpu().numpy() != w_rank)[0][:10]
    bad = np.nonzero(matched.cpu().numpy() != w_matched)[0]
    assert bad.size == 0, (bad[:10], matched.cpu().numpy()[bad[:3]], w_matched[bad[:3]])
    bad = np.nonzero(ignored.cpu().numpy() != w_ignored)[0]
    assert bad.size == 0, (bad[:10], ignored.cpu().numpy()[bad[:3]], w_ignored[bad[:3]])
    assert np.array_equal(npig.cpu().numpy(), w_npig)
    assert np.array_equal(present.cpu().numpy(), w_present)
    assert w_matched.any() and w_ignored.any()


def test_match_flags_a_label_outside_the_range_and_refuses_bad_offsets():
    case = [dc.image([[0, 0, 10, 10], [5, 5, 30, 30]], [0.9, 0.8], [3, 256], [[0, 0, 10, 10]], [3]),
            dc.image([[0, 0, 10, 10]], [0.9], [-1], [[0, 0, 10, 10]], [3])]
    rank, matched, ignored, npig, present, flag = _match(case)
    assert int(flag.cpu()) == 1
    assert rank.cpu().tolist() == [0, 1024, 1024] and int(matched[0].cpu()) != 0 and matched[1:].cpu().tolist() == [0, 0]
    assert present.cpu().nonzero().squeeze(1).tolist() == [3] and int(npig[3, 0].cpu()) == 2
    args = list(dc.flat(case, DEV))
    args[3] = torch.tensor([0, 2, 9], dtype=torch.int32, device=DEV)      # past the end of the detections
    assert int(_ops().det_map_match(*args)[5].cpu()) & 2


def _order_ref(scores, labels, rank):
    idx = np.nonzero(rank < 100)[0]
    idx = idx[np.argsort(-scores[idx], kind="mergesort")]
    idx = idx[np.argsort(labels[idx], kind="mergesort")]
    seg = np.concatenate([[0], np.cumsum(np.bincount(labels[idx], minlength=256))])
    return idx, seg


@pytest.mark.parametrize("n", (1, 255, 256, 257, 4095, 4096, 4097, 5000, 20000))
def test_order_is_the_stable_sort_by_label_and_descending_score(n):
    rng = np.random.default_rng(n)
    scores = (np.round(rng.random(n) * 64) / 64).astype(np.float32)           # many ties
    scores[rng.random(n) < 0.1] *= -1                                        # the sign flips the bit pattern's order
    scores[rng.random(n) < 0.05] = -0.0                                      # -0 ties with +0
    labels = rng.choice([0, 1, 7, 128, 255], n).astype(np.int64)
    rank = rng.integers(0, 125, n).astype(np.int32)
    want, seg = _order_ref(scores, labels, rank)
    got, got_seg = _ops().det_map_order(torch.from_numpy(scores).to(DEV), torch.from_numpy(labels).to(DEV),
                                        torch.from_numpy(rank).to(DEV))
    assert np.array_equal(got_seg.cpu().numpy(), seg)
    assert np.array_equal(got.cpu().numpy()[:len(want)], want)


def test_order_is_stable_on_one_shared_score_and_label():
    n = 5000
    scores = torch.full((n,), 0.25, device=DEV)
    labels = torch.full((n,), 9, dtype=torch.int64, device=DEV)
    got, seg = _ops().det_map_order(scores, labels, torch.zeros(n, dtype=torch.int32, device=DEV))
    assert torch.equal(got.cpu(), torch.arange(n, dtype=torch.int32))
    assert seg.cpu().tolist() == [0] * 10 + [n] * 247


COMBOS = ((0, 2), (1, 2), (2, 2), (3, 2), (0, 0), (0, 1))    # (area, maxDet index) of the six pairs


@pytest.mark.parametrize("name", ("segments", "random1"))
def test_accumulate_precision_sums_and_recalls(name):
    ops = _ops()
    case = _case(name)
    det = dc.flat(case, DEV)
    rank, matched, ignored, npig, present, flag = ops.det_map_match(*det)
    sorted_idx, seg_off = ops.det_map_order(det[1], det[2], rank)
    stats, out64, out32, outi = ops.det_map_accumulate(sorted_idx, seg_off, rank, matched, ignored, npig, present, flag)
    precision, recall, classes, summary = _restated(name)
    stats = stats.cpu().numpy()
    if name == "segments":
        seg = np.diff(seg_off.cpu().numpy())
        assert seg[:7].tolist() == [0, 1, 255, 256, 257, 513, 40] and int(npig[6].sum().cpu()) == 0
    head = outi.cpu().tolist()
    assert head[0] == len(classes) and head[1] == 0 and head[2:2 + head[0]] == classes
    for k, c in enumerate(classes):
        for j, (a, m) in enumerate(COMBOS):
            want_p, want_r = precision[:, :, k, a, m].sum(1), recall[:, k, a, m]
            if (want_r == -1).all():
                assert (stats[c, j] == -1).all(), (c, j)
                continue
            assert (want_r > -1).all()
            assert np.abs(stats[c, j, :, 0] - want_p).max() < 1e-9, (c, j, stats[c, j, :, 0], want_p)
            assert np.abs(stats[c, j, :, 1] - want_r).max() < 1e-12, (c, j, stats[c, j, :, 1], want_r)
    for i, key in enumerate(dc.NAMES):
        assert abs(float(out64[i].cpu()) - summary[key]) < 1e-9, (key, float(out64[i].cpu()), summary[key])
    assert torch.equal(out32.cpu(), out64.cpu().float())


def _metric(case, splits=1, device=DEV):
    from ssl4gie_amd import metrics
    m = metrics.MeanAveragePrecision()
    preds, target = dc.to_updates(case, device)
    step = -(-len(preds) // splits)
    for s in range(0, len(preds), step):
        m.update(preds[s:s + step], target[s:s + step])
    return m


@pytest.mark.parametrize("name", ("docstring", "random1", "random2", "shape3", "exact", "rounding"))
def test_end_to_end_against_the_restatement(name, monkeypatch):
    case = _case(name)
    summary, classes = _restated(name)[3], _restated(name)[2]
    m = _metric(case)
    f64, res = m.compute_f64(), m.compute()
    for key in dc.NAMES:
        assert f64[key].dtype == torch.float64 and f64[key].dim() == 0 and f64[key].is_cuda
        assert abs(float(f64[key]) - summary[key]) < 1e-9, (key, float(f64[key]), summary[key])
        assert res[key].dtype == torch.float32 and res[key].dim() == 0 and res[key].is_cuda
        assert float(res[key]) == float(torch.tensor(float(f64[key]), dtype=torch.float64).float())
    assert res["classes"].dtype == torch.int32 and res["classes"].cpu().tolist() == classes
    assert float(res["map_per_class"]) == -1.0 and float(res["mar_100_per_class"]) == -1.0
    # the same data in several updates: the same bits
    for splits in (3, len(case)):
        again = _metric(case, splits).compute_f64()
        assert all(float(again[k]) == float(f64[k]) for k in dc.NAMES)
    if name in ("docstring", "random1"):
        monkeypatch.setenv("SSL4GIE_FUSED_METRICS", "0")
        plain = _metric(case).compute_f64()
        assert all(abs(float(plain[k]) - float(f64[k])) < 1e-9 for k in dc.NAMES)


def test_docstring_example_values_reset_and_label_check():
    from ssl4gie_amd import metrics
    m = _metric(_case("docstring"))
    res = {k: float(v) for k, v in m.compute().items() if k != "classes"}
    six = float(torch.tensor(0.6))
    assert res["map"] == six and res["map_50"] == 1.0 and res["map_75"] == 1.0 and res["map_large"] == six
    assert res["map_small"] == -1.0 and res["map_medium"] == -1.0
    assert res["mar_1"] == res["mar_10"] == res["mar_100"] == res["mar_large"] == six
    m.reset()
    empty = m.compute()
    assert all(float(empty[k]) == -1.0 for k in dc.NAMES) and empty["classes"].numel() == 0
    m.update(*dc.to_updates(_case("random1"), DEV))
    want = _restated("random1")[3]
    assert abs(float(m.compute_f64()["map"]) - want["map"]) < 1e-9
    # ground truths without any detection, detections without any ground truth
    only_gt = _metric([dc.image(gt_boxes=[[0, 0, 50, 50]], gt_labels=[2])]).compute()
    assert float(only_gt["map"]) == 0.0 and float(only_gt["mar_100"]) == 0.0 and float(only_gt["map_small"]) == -1.0
    only_det = _metric([dc.image([[0, 0, 50, 50]], [0.5], [2])]).compute()
    assert float(only_det["map"]) == -1.0 and only_det["classes"].cpu().tolist() == [2]
    bad = metrics.MeanAveragePrecision()
    bad.update(*dc.to_updates([dc.image([[0, 0, 5, 5]], [0.5], [256], [[0, 0, 5, 5]], [1])], DEV))
    with pytest.raises(ValueError):
        bad.compute()
