"""GPU: ssl4gie_det_color / ssl4gie_det_geometry / ssl4gie_det_boxes against the restatement of their rule
(tests/det_input_checks.py, pinned on the CPU by tests/test_det_input_checks_cpu.py) and against the reference's own
dataset class (tests/golden/g21_det_loader.npz), their exactness properties and guards, and DetectionTransform through
the DetectionLoader.

Exact: without a halving the geometry only moves float(v) / 255 values, so images are compared bit for bit; box
arithmetic is the reference's float32 statements, so boxes are compared bit for bit everywhere.
Halved images: the bar is 4 x the largest error of torch's own float32 CPU F.interpolate against the float64
restatement on the same inputs, computed here and printed.  Colour stage: 4 x the largest error of the restatement's
own float32 CPU evaluation against its float64 evaluation on the same rows — test_gpu_color_augment.py's convention.
No case excludes a pixel or a box."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import colour_checks as cc
import det_input_checks as dc
import warp_checks as wc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
G21 = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g21_det_loader.npz")
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


@pytest.fixture(scope="module", autouse=True)
def _lib_loaded():
    from ssl4gie_amd import _lib
    _lib.load()


def bits(t):
    return np.ascontiguousarray(t.detach().cpu().numpy() if torch.is_tensor(t) else np.asarray(t, np.float32)).view(np.uint32)


def make_bank(images, boxes=None):
    from ssl4gie_amd.data import RaggedImageBank
    boxes = [np.zeros((0, 4), np.float32)] * len(images) if boxes is None else boxes
    return RaggedImageBank.from_arrays([np.ascontiguousarray(i) for i in images], boxes, DEV)


def dev_index(idx):
    return torch.tensor(idx, dtype=torch.int64, device=DEV)


def dev_geom(decs):
    return torch.tensor([dc.geom_bits(d) for d in decs], dtype=torch.uint8, device=DEV)


def skip_rows(B):
    """a colour stage that changes nothing: every op skipped, no blur"""
    return (torch.tensor([[1.0, 1.0, 1.0, 0.0]] * B, device=DEV), torch.full((B, 4), 255, dtype=torch.uint8, device=DEV),
            torch.zeros(B, device=DEV))


def geometry(bank, idx, decs, F, mean=cc.ZERO3, std=cc.ONE3, color=None):
    """color: None = the eval path (uint8 source); (factors, order, sigma) = the training path through the scratch"""
    from ssl4gie_amd import ops
    index, scratch = dev_index(idx), None
    if color is not None:
        inside = [i for i in idx if 0 <= i < len(bank)]
        max_hw = (max(bank.sizes_host[i][0] for i in inside), max(bank.sizes_host[i][1] for i in inside))
        scratch = ops.det_color(bank.pixels, bank.offsets, bank.sizes, index, *color, max_hw)
    return ops.det_geometry(bank.pixels, bank.offsets, bank.sizes, index, dev_geom(decs), F, mean, std, scratch)


def run_boxes(bank, idx, decs, F, counts=None):
    from ssl4gie_amd import ops
    off = bank.box_offsets_host
    counts = [off[i + 1] - off[i] for i in idx] if counts is None else counts
    starts = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    out, labels = ops.det_boxes(bank.boxes, bank.box_labels, bank.box_offsets, bank.sizes, dev_index(idx), dev_geom(decs),
                                torch.from_numpy(starts).to(DEV), int(starts[-1]), max(counts), F)
    return out.cpu(), labels.cpu(), starts


@pytest.fixture(scope="module")
def fixture_bank():
    cases, F = dc.g21(G21)
    return cases, F, make_bank([c[0] for c in cases], [c[1] for c in cases])


# ---- exact cases -----------------------------------------------------------------------------------------------------
def test_every_fixture_case_through_the_eval_path(fixture_bank):
    cases, F, bank = fixture_bank
    idx, decs = list(range(len(cases))), [c[2] for c in cases]
    got = geometry(bank, idx, decs, F).cpu()
    n_exact, halved = 0, []
    for k, (img, _, dec, out_img, _) in enumerate(cases):
        if not dc.is_halved(img, dec, F):
            n_exact += 1
            assert np.array_equal(bits(got[k]), bits(out_img)), (img.shape, dec)
            continue
        ref64, err32 = dc.halved_ref_and_err32(img, dec, F)
        err = float((got[k].to(torch.float64) - ref64).abs().max())
        err_fixture = float((got[k].to(torch.float64) - torch.from_numpy(out_img).to(torch.float64)).abs().max())
        print(f"halved {img.shape[:2]} {dec}: max |kernel - fp64| = {err:.3e}, torch's float32 interpolate {err32:.3e}; "
              f"|kernel - reference's float32 image| = {err_fixture:.3e}")
        assert bool((got[k][ref64 == 0.0] == 0.0).all())     # the pads are exact zeros
        halved.append((err, err32, img.shape[:2], dec))
    bar = 4.0 * max(h[1] for h in halved)
    print(f"bar = 4 x the largest float32 interpolate error = {bar:.3e}; largest kernel error {max(h[0] for h in halved):.3e}")
    assert n_exact == 3 and len(halved) == 11
    for err, _, shape, dec in halved:
        assert err <= bar, (shape, dec, err, bar)


def test_every_fixture_box_is_bit_equal(fixture_bank):
    cases, F, bank = fixture_bank
    idx, decs = list(range(len(cases))), [c[2] for c in cases]
    out, labels, starts = run_boxes(bank, idx, decs, F)
    assert labels.tolist() == [1] * int(starts[-1])
    for k, c in enumerate(cases):
        got = out[starts[k]:starts[k + 1]]
        assert got.shape == c[4].shape and np.array_equal(bits(got), bits(c[4])), (c[0].shape, c[2])
        assert np.array_equal(bits(got), bits(dc.boxes_ref(c[1], c[0].shape[0], c[0].shape[1], c[2], F)))


def test_eval_path_equals_training_geometry_with_the_colour_stage_skipped(fixture_bank):
    cases, F, bank = fixture_bank
    idx, decs = list(range(len(cases))), [c[2] for c in cases]
    a = geometry(bank, idx, decs, F)
    b = geometry(bank, idx, decs, F, color=skip_rows(len(idx)))
    assert torch.equal(a.view(torch.int32), b.view(torch.int32))


def some_color(B):
    factors = torch.tensor([[1.3, 0.7, 1.2, 0.01], [0.7, 1.4, 0.8, -0.01]] * B, device=DEV)[:B].contiguous()
    order = torch.tensor([[2, 1, 0, 3], [3, 0, 1, 2]] * B, dtype=torch.uint8, device=DEV)[:B].contiguous()
    return factors, order, torch.tensor([2.0, 0.7] * B, device=DEV)[:B].contiguous()


def test_alone_and_as_one_of_five_and_twice(fixture_bank):
    cases, F, bank = fixture_bank
    idx, decs = [8, 0, 12, 5, 10], [cases[i][2] for i in (8, 0, 12, 5, 10)]
    f, o, s = some_color(5)
    five = geometry(bank, idx, decs, F, MEAN, STD, (f, o, s))
    again = geometry(bank, idx, decs, F, MEAN, STD, (f, o, s))
    assert torch.equal(five.view(torch.int32), again.view(torch.int32))
    for pos in (3, 4):   # a halved 71 x 93 with sigma 0.7 and a halved 100 x 50 with sigma 2
        alone = geometry(bank, [idx[pos]], [decs[pos]], F, MEAN, STD, (f[pos:pos + 1], o[pos:pos + 1], s[pos:pos + 1]))
        assert torch.equal(alone[0].view(torch.int32), five[pos].view(torch.int32)), pos
    b5, _, st = run_boxes(bank, idx, decs, F)
    b1, _, _ = run_boxes(bank, [idx[4]], [decs[4]], F)
    assert b1.shape == (3, 4) and np.array_equal(bits(b5[st[4]:st[5]]), bits(b1))


def test_normalisation_and_padding(fixture_bank):
    cases, F, bank = fixture_bank
    idx, decs = list(range(len(cases))), [c[2] for c in cases]
    plain = geometry(bank, idx, decs, F).cpu()
    normed = geometry(bank, idx, decs, F, MEAN, STD).cpu()
    m, s = torch.tensor(MEAN).view(1, 3, 1, 1), torch.tensor(STD).view(1, 3, 1, 1)
    want = (plain - m) / s
    ulp = torch.maximum(want.abs(), torch.tensor(2.0 ** -126)) * 2.0 ** -23    # >= the spacing of float32 at `want`
    assert bool(((normed - want).abs() <= ulp).all())
    black = ((torch.zeros(1, 3, 1, 1) - m) / s).expand_as(normed)
    for k, (img, _, dec, _, _) in enumerate(cases):
        _, _, _, H2, W2, p1, p2 = dc.out_geometry(img.shape[0], img.shape[1], dec[0], F)
        pad = torch.ones(F, F, dtype=torch.bool)
        pad[p2:p2 + H2, p1:p1 + W2] = False
        assert torch.equal(normed[k][:, pad], black[k][:, pad]), k


# ---- the colour stage on rectangles ----------------------------------------------------------------------------------
def color_scratch(u8, factors, order, sigma):
    from ssl4gie_amd import ops
    B, H, W = u8.shape[:3]
    bank = make_bank(list(u8))
    s = ops.det_color(bank.pixels, bank.offsets, bank.sizes, dev_index(list(range(B))), factors.to(DEV), order.to(DEV),
                      sigma.to(DEV), (H, W))
    return s[:, :, :H * W].reshape(B, 3, H, W).cpu()


@pytest.mark.parametrize("H,W", dc.COLOR_SHAPES)
def test_colour_stage_on_rectangles(H, W):
    """all 24 orders, a skip row, sigma in {0, 0.001, 0.34, 1, 2}; at 13 x 13 and 16 x 40 every halo is reflected"""
    u8, factors, order, sigma, ref64, err32 = dc.color_case(H, W)
    got = color_scratch(u8, factors, order, sigma)
    assert bool(torch.isfinite(got).all())
    d = (got.to(torch.float64) - ref64).abs()
    err, bar = float(d.max()), 4.0 * err32
    worst = int(d.flatten(1).max(dim=1).values.argmax())
    print(f"det_color {H} x {W}: max |kernel - fp64| = {err:.3e} (row {worst}: order {order[worst].tolist()}, sigma "
          f"{float(sigma[worst]):.3f}), float32 CPU evaluation {err32:.3e}, bar {bar:.3e}")
    assert err <= bar
    tiny = torch.where(sigma == 0.0, torch.tensor(0.001), sigma)
    none = torch.where(sigma == 0.001, torch.tensor(0.0), sigma)
    a, b = color_scratch(u8, factors, order, tiny), color_scratch(u8, factors, order, none)
    assert torch.equal(a.view(torch.int32), b.view(torch.int32)) and torch.equal(a.view(torch.int32), got.view(torch.int32))


# ---- production shape ------------------------------------------------------------------------------------------------
def test_production_shape():
    """B = 2, F = 1024: a 1072 x 1920 image, rotated to 1920 x 1072, halved to 960 x 536 and padded, its colour stage a
    no-op through the scratch; and a 487 x 332 image, not halved, with the full colour stage (16 x 6 tiles: the blur
    crosses tile seams inside the image)"""
    F = 1024
    g = np.random.default_rng(11)
    yy, xx = np.meshgrid(np.arange(1072) / 1072, np.arange(1920) / 1920, indexing="ij")
    big = np.clip(np.stack([180 * xx, 180 * yy, 90 + 90 * np.sin(9 * xx + 5 * yy)], 2) + g.integers(0, 60, (1072, 1920, 3)),
                  0, 255).astype(np.uint8)
    small = g.integers(0, 256, (487, 332, 3), dtype=np.uint8)
    boxes = [np.array([[100.5, 200.25, 1800.0, 1000.75]], np.float32), np.array([[3.0, 4.0, 300.0, 480.0]], np.float32)]
    bank = make_bank([big, small], boxes)
    decs = [(1, 0, 1), (0, 1, 0)]
    factors = torch.tensor([[1.0, 1.0, 1.0, 0.0], [1.3, 0.7, 1.2, 0.01]], device=DEV)
    order = torch.tensor([[255] * 4, [2, 1, 0, 3]], dtype=torch.uint8, device=DEV)
    sigma = torch.tensor([0.0, 2.0], device=DEV)
    got = geometry(bank, [0, 1], decs, F, color=(factors, order, sigma)).cpu()

    ref_big, err32_big = dc.halved_ref_and_err32(big, decs[0], F)
    bar_big = 4.0 * err32_big
    err_big = float((got[0].to(torch.float64) - ref_big).abs().max())
    x = dc.to_tensor(small).unsqueeze(0)
    rows = (factors[1:].cpu(), order[1:].cpu(), sigma[1:].cpu())
    c64, c32 = dc.color_rect_ref(x, *rows, torch.float64), dc.color_rect_ref(x, *rows, torch.float32)
    bar_small = 4.0 * float((c32.to(torch.float64) - c64).abs().max())
    err_small = float((got[1].to(torch.float64) - dc.geometry_ref(c64[0], decs[1], F)).abs().max())
    print(f"production: 1072 x 1920 halved: max |kernel - fp64| = {err_big:.3e}, bar {bar_big:.3e}; 487 x 332 coloured: "
          f"{err_small:.3e}, bar {bar_small:.3e}")
    assert err_big <= bar_big and err_small <= bar_small
    out, _, st = run_boxes(bank, [0, 1], decs, F)
    for k in (0, 1):
        assert np.array_equal(bits(out[st[k]:st[k + 1]]), bits(dc.boxes_ref(boxes[k], *bank.sizes_host[k], decs[k], F)))


# ---- guards ----------------------------------------------------------------------------------------------------------
def test_bad_index_gives_nan_sample_and_nan_boxes(fixture_bank):
    cases, F, bank = fixture_bank
    n = len(bank)
    idx, decs = [10, n, 3], [cases[10][2], (1, 0, 0), cases[3][2]]
    f, o, s = some_color(3)
    for color in (None, (f, o, s)):
        got = geometry(bank, idx, decs, F, color=color)
        good = geometry(bank, [10, 3], [decs[0], decs[2]], F, color=None if color is None else (f[[0, 2]], o[[0, 2]], s[[0, 2]]))
        assert bool(torch.isnan(got[1]).all())
        assert torch.equal(got[[0, 2]].view(torch.int32), good.view(torch.int32))
    out, labels, st = run_boxes(bank, idx, decs, F, counts=[len(cases[10][1]), 2, len(cases[3][1])])
    assert len(cases[10][1]) == 3 and len(cases[3][1]) == 3
    assert bool(torch.isnan(out[3:5]).all()) and labels[3:5].tolist() == [-1, -1]
    assert np.array_equal(bits(out[0:3]), bits(cases[10][4])) and np.array_equal(bits(out[5:8]), bits(cases[3][4]))
    assert labels[0:3].tolist() == [1, 1, 1] and labels[5:8].tolist() == [1, 1, 1]


def test_every_refusal_returns_before_a_launch(fixture_bank):
    from ssl4gie_amd import _lib
    from ssl4gie_amd.ops import ptr, stream
    L = _lib.load()
    cases, F, bank = fixture_bank
    B = 2
    index, geom = dev_index([0, 9]), dev_geom([(0, 0, 0), (1, 0, 0)])
    out = torch.full((B * 3 * F * F + 4,), 7.0, device=DEV)
    f, o, s = some_color(B)
    stride = bank.max_pixels + 3 & ~3
    scratch = torch.full((B * 3 * stride + 4,), 7.0, device=DEV)
    ws = torch.empty(L.ssl4gie_det_color_workspace_bytes(B), dtype=torch.uint8, device=DEV)
    m1, s1 = (C.c_float * 3)(0, 0, 0), (C.c_float * 3)(1, 1, 1)
    s0 = (C.c_float * 3)(1, 0, 1)

    def geo(pix=ptr(bank.pixels), offs=ptr(bank.offsets), sizes=ptr(bank.sizes), idx=ptr(index), o_=ptr(out), F_=F, std=s1,
            mean=m1, scr=0):
        return L.ssl4gie_det_geometry(scr, stride if scr else 0, pix, bank.pixels.numel(), offs, sizes, len(bank), idx,
                                      ptr(geom), o_, B, F_, mean, std, stream())

    def col(pix=ptr(bank.pixels), fac=ptr(f), scr=ptr(scratch), w=ptr(ws), wb=ws.numel(), sig=ptr(s)):
        return L.ssl4gie_det_color(pix, bank.pixels.numel(), ptr(bank.offsets), ptr(bank.sizes), len(bank), ptr(index), B,
                                   128, 128, fac, ptr(o), sig, scr, stride, w, wb, stream())

    bx = torch.full((8 * 4 + 4,), 7.0, device=DEV)
    lab = torch.zeros(8, dtype=torch.int64, device=DEV)
    start = torch.tensor([0, 3, 4], dtype=torch.int64, device=DEV)

    def box(b=ptr(bank.boxes), ob=ptr(bx), st=ptr(start), F_=F):
        return L.ssl4gie_det_boxes(b, ptr(bank.box_labels), ptr(bank.box_offsets), bank.boxes.shape[0], ptr(bank.sizes),
                                   len(bank), ptr(index), ptr(geom), st, ob, ptr(lab), 4, B, F_, 3, stream())

    refused = [geo(pix=0), geo(offs=0), geo(sizes=0), geo(idx=0), geo(o_=0), geo(mean=None), geo(std=None), geo(F_=F + 2),
               geo(std=s0), geo(o_=ptr(out) + 4), geo(scr=ptr(scratch) + 4),
               col(pix=0), col(fac=0), col(sig=0), col(scr=0), col(w=0), col(wb=ws.numel() - 1), col(scr=ptr(scratch) + 4),
               box(b=0), box(ob=0), box(st=0), box(F_=F + 2), box(ob=ptr(bx) + 4)]
    torch.cuda.synchronize()
    assert refused == [1000] * len(refused), refused    # SSL4GIE_EARG
    assert bool((out == 7.0).all()) and bool((scratch == 7.0).all()) and bool((bx == 7.0).all())   # nothing was written
    assert geo() == 0 and col() == 0 and box() == 0
    torch.cuda.synchronize()


# ---- end to end ------------------------------------------------------------------------------------------------------
def test_detection_loader_end_to_end(fixture_bank):
    from ssl4gie_amd.data import DetectionLoader, DetectionTransform
    cases, F, _ = fixture_bank
    pick = [0, 8, 9, 10, 11, 12, 13]                       # the seven shapes
    imgs, boxes = [cases[i][0] for i in pick], [cases[i][1] for i in pick]
    bank = make_bank(imgs, boxes)
    gen = torch.Generator(device=DEV).manual_seed(2024)
    tf = DetectionTransform(F, mean=MEAN, std=STD, generator=gen)
    loader = DetectionLoader(bank, 3, sampler=torch.utils.data.SequentialSampler(bank), drop_last=False, transform=tf)
    assert len(loader) == 3
    seen, errs = 0, []
    for images, targets in loader:
        B = len(images)
        assert isinstance(images, tuple) and isinstance(targets, tuple) and len(targets) == B and B in (3, 1)
        stacked = loader.last_images
        assert tuple(stacked.shape) == (B, 3, F, F) and stacked.dtype == torch.float32
        factors, order, sigma, geom = (t.cpu() for t in tf.last_draw)
        row = 0
        for b in range(B):
            k = seen + b
            assert tuple(images[b].shape) == (3, F, F) and images[b].data_ptr() == stacked[b].data_ptr()
            assert images[b].cuda(0) is images[b]
            t = targets[b]
            assert set(t) == {"boxes", "labels"} and t["labels"].dtype == torch.int64
            assert tuple(t["boxes"].shape) == (len(boxes[k]), 4) and t["labels"].tolist() == [1] * len(boxes[k])
            if len(boxes[k]):
                assert t["boxes"].data_ptr() == loader.last_boxes[row:].data_ptr()
            row += len(boxes[k])
            dec = dc.bits_dec(int(geom[b]))
            H0, W0 = imgs[k].shape[:2]
            assert np.array_equal(bits(t["boxes"]), bits(dc.boxes_ref(boxes[k], H0, W0, dec, F)))
            # the whole restatement in float64, and in float32 with torch's own F.interpolate as the halving
            x = dc.to_tensor(imgs[k]).unsqueeze(0)
            rows = (factors[b:b + 1], order[b:b + 1], sigma[b:b + 1])
            c64, c32 = dc.color_rect_ref(x, *rows, torch.float64)[0], dc.color_rect_ref(x, *rows, torch.float32)[0]
            ref64 = dc.geometry_ref(c64, dec, F, mean=MEAN, std=STD)
            t32 = dc.turned(c32, dec)
            if dc.out_geometry(H0, W0, dec[0], F)[2]:
                t32 = torch.nn.functional.pad(t32, (0, t32.shape[2] % 2, 0, t32.shape[1] % 2))
                t32 = torch.nn.functional.interpolate(t32.unsqueeze(0), size=(t32.shape[1] // 2, t32.shape[2] // 2),
                                                      mode="bicubic", antialias=True, align_corners=False)[0]
            _, _, _, H2, W2, p1, p2 = dc.out_geometry(H0, W0, dec[0], F)
            inside = ref64[:, p2:p2 + H2, p1:p1 + W2]
            m32, s32 = torch.tensor(MEAN).view(3, 1, 1), torch.tensor(STD).view(3, 1, 1)
            err32 = float((((t32 - m32) / s32).to(torch.float64) - inside).abs().max())
            err = float((images[b].cpu().to(torch.float64) - ref64).abs().max())
            print(f"loader sample {k} ({H0} x {W0}, dec {dec}, sigma {float(sigma[b]):.3f}): max |kernel - fp64| = {err:.3e}, "
                  f"float32 CPU evaluation {err32:.3e}")
            errs.append((err, err32))
        seen += B
    assert seen == 7
    bar = 4.0 * max(e[1] for e in errs)
    print(f"bar = 4 x the largest float32 CPU evaluation error = {bar:.3e}; largest kernel error {max(e[0] for e in errs):.3e}")
    assert all(e[0] <= bar for e in errs), (errs, bar)
    # the same seed draws the same batches
    tf2 = DetectionTransform(F, mean=MEAN, std=STD, generator=torch.Generator(device=DEV).manual_seed(2024))
    first = next(iter(DetectionLoader(bank, 3, sampler=torch.utils.data.SequentialSampler(bank), transform=tf2)))
    again = next(iter(DetectionLoader(bank, 3, sampler=torch.utils.data.SequentialSampler(bank), transform=DetectionTransform(
        F, mean=MEAN, std=STD, generator=torch.Generator(device=DEV).manual_seed(2024)))))
    assert all(torch.equal(a, b) for a, b in zip(first[0], again[0]))


def test_scratch_is_sized_by_pixels_not_by_the_batch_bounding_rectangle():
    """a tall and a wide image in one batch: max H x max W of the batch exceeds the largest image"""
    from ssl4gie_amd.data import DetectionTransform
    imgs = [np.random.default_rng(k).integers(0, 256, s, dtype=np.uint8) for k, s in enumerate(((100, 14, 3), (13, 93, 3)))]
    bank = make_bank(imgs)
    tf = DetectionTransform(64, brightness=0.0, contrast=0.0, saturation=0.0, hue=0.0, blur_sigma=(0.001, 0.002),
                            rotate=False, hflip=False, vflip=False)
    images, boxes, labels = tf(bank, dev_index([0, 1]))
    assert tuple(tf._scratch.shape) == (2, 3, 1400) and tuple(boxes.shape) == (0, 4) and tuple(labels.shape) == (0,)
    want = geometry(bank, [0, 1], [(0, 0, 0)] * 2, 64)                 # nothing jittered, nothing blurred: the eval bits
    assert torch.equal(images.view(torch.int32), want.view(torch.int32))


def test_eval_transform(fixture_bank):
    """the val / test loader: no draw is ever true; un-halved images and all boxes equal the restatement's bits"""
    from ssl4gie_amd.data import DetectionLoader, DetectionTransform
    cases, F, bank = fixture_bank
    loader = DetectionLoader(bank, 1, sampler=torch.utils.data.SequentialSampler(bank), drop_last=False,
                             transform=DetectionTransform.eval(F))
    n = 0
    for k, (images, targets) in enumerate(loader):
        img, b = cases[k][0], cases[k][1]
        if not dc.is_halved(img, (0, 0, 0), F):
            n += 1
            assert np.array_equal(bits(images[0]), bits(dc.geometry_ref(dc.to_tensor(img), (0, 0, 0), F)))
        assert np.array_equal(bits(targets[0]["boxes"]), bits(dc.boxes_ref(b, img.shape[0], img.shape[1], (0, 0, 0), F)))
    assert n == 3
