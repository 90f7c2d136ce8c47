"""GPU: the RandAugment / RandomErasing kernels (ssl4gie_quantize_u8, ssl4gie_randaug_layer,
ssl4gie_normalize_erase_u8) against the numpy restatements of tests/randaug_checks.py — which
tests/test_randaug_checks_cpu.py holds to PIL bit for bit, so no PIL is needed here — and MAEFinetuneTransform through
DeviceLoader.  The uint8 stages are compared byte for byte with no mask.  The noise inside an erased box is compared
with the fp64 Box-Muller of the restated integers; its bar is 4 x the error of the restatement's own float32 CPU
evaluation against fp64 on the same values, computed and printed here (the suite's convention)."""
import numpy as np
import pytest
import torch

import randaug_checks as rc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module", autouse=True)
def _lib_loaded():
    from ssl4gie_amd import _lib
    _lib.load()


def _clone(g):
    g2 = torch.Generator(device=DEV)
    g2.set_state(g.get_state())
    return g2


def _layer(imgs, op, arg, matrix, fill=rc.FILL):
    from ssl4gie_amd import ops
    out = ops.randaug_layer(torch.from_numpy(imgs).to(DEV), torch.from_numpy(op).to(DEV), torch.from_numpy(arg).to(DEV),
                            torch.from_numpy(np.ascontiguousarray(matrix)).to(DEV), fill)
    return out.cpu().numpy()


def _same(got, want, names):
    assert got.dtype == np.uint8 and got.shape == want.shape
    bad = [(names[b], int((got[b] != want[b]).sum())) for b in range(got.shape[0]) if not np.array_equal(got[b], want[b])]
    assert not bad, bad


@pytest.mark.parametrize("S", [16, 36])
def test_layer_is_the_restatement_byte_for_byte_on_the_fixed_cases(S):
    """every op id with the arguments of op_cases(S), one launch.  S = 16: one workgroup per sample, 16 units; S = 36:
    81 units = 243 chunks, no multiple of the wave size"""
    cases = rc.op_cases(S)
    imgs, op, arg, matrix = rc.layer_batch(S, cases)
    assert set(op.tolist()) == set(range(rc.N_OPS))
    _same(_layer(imgs, op, arg, matrix), rc.layer_ref(imgs, op, arg, matrix), [c[0] for c in cases])


def _production_rows():
    """(op, arg, matrix) per id at the recipe's magnitude 9 (inc1), S = 224"""
    S, rows = 224, []
    for o in range(rc.N_OPS):
        a = rc.timm_level_arg(o, 9.0, o % 2 == 1, 1, S)
        rows.append((o, 0.0 if a is None else a, rc.op_matrix(o, a, S) if o in rc.GEOMETRIC else rc.IDENTITY))
    return rows


@pytest.fixture(scope="module")
def production_images():
    return np.stack([rc.image(224, 0, "smooth"), rc.image(224, 1, "noise")])


@pytest.mark.parametrize("first", range(0, rc.N_OPS + 1, 2))
def test_layer_production_grid(first, production_images):
    """B = 2 at S = 224 (13 workgroups per sample, the last one partial), two op ids per launch; the last pair is
    TranslateYRel with a skipped sample"""
    rows = _production_rows() + [(rc.SKIP, 0.0, rc.IDENTITY)]
    pair = rows[first:first + 2]
    op = np.array([r[0] for r in pair], dtype=np.uint8)
    arg = np.array([r[1] for r in pair], dtype=np.float32)
    matrix = np.array([r[2] for r in pair], dtype=np.float64)
    got = _layer(production_images, op, arg, matrix)
    _same(got, rc.layer_ref(production_images, op, arg, matrix), [f"op {int(o)}" for o in op])


def test_layer_mixed_batch_skip_and_unknown_ids_copy():
    S = 36
    ids = list(range(rc.N_OPS)) + [rc.SKIP, 15, 200]
    imgs = np.stack([rc.image(S, i, "noise" if i % 2 else "smooth") for i in range(len(ids))])
    op = np.array(ids, dtype=np.uint8)
    arg = np.array([0, 0, 0, 12.5, 2, 77, 60, 1.6, 0.4, 1.3, 1.9, 0.2, -0.2, 5.5, -7.25, 3, 3, 3], dtype=np.float32)
    matrix = np.array([rc.op_matrix(o, a, S) for o, a in zip(ids, arg)], dtype=np.float64)
    matrix[-3:] = np.nan    # a copy reads no matrix
    got = _layer(imgs, op, arg, matrix)
    _same(got, rc.layer_ref(imgs, op, arg, matrix), [f"op {o}" for o in ids])
    assert np.array_equal(got[-3:], imgs[-3:])


def test_layer_nan_matrix_row_fills_its_sample_only():
    S = 20
    imgs = np.stack([rc.image(S, i) for i in range(3)])
    op = np.full(3, rc.ROTATE, dtype=np.uint8)
    arg = np.zeros(3, dtype=np.float32)
    matrix = np.array([rc.rotate_matrix(20.0, S), (np.nan,) * 6, rc.rotate_matrix(-11.0, S)], dtype=np.float64)
    got = _layer(imgs, op, arg, matrix)
    assert (got[1] == np.array(rc.FILL, np.uint8)).all()
    _same(got, rc.layer_ref(imgs, op, arg, matrix), ["20 deg", "NaN", "-11 deg"])
    matrix[1] = (1e300, -1e300, 1e308, 3.0, 1e200, -1e308)    # enormous coefficients fill too, or clamp: no fault
    _same(_layer(imgs, op, arg, matrix), rc.layer_ref(imgs, op, arg, matrix), ["20 deg", "huge", "-11 deg"])


def test_layer_on_a_bank_read_through_a_permuted_index():
    S, n = 16, 6
    bank = np.stack([rc.image(S, i) for i in range(n)])
    perm = np.array([4, 0, 5, 2, 2, 1])
    op = np.array([rc.EQUALIZE, rc.SHARPNESS, rc.SHEAR_X, rc.COLOR, rc.CONTRAST, rc.AUTO_CONTRAST], dtype=np.uint8)
    arg = np.array([0, 1.7, 0.25, 0.3, 1.45, 0], dtype=np.float32)
    matrix = np.array([rc.op_matrix(o, a, S) for o, a in zip(op, arg)], dtype=np.float64)
    from ssl4gie_amd import ops
    dev_bank = torch.from_numpy(bank).to(DEV)
    got = ops.randaug_layer(dev_bank[torch.from_numpy(perm).to(DEV)], torch.from_numpy(op).to(DEV),
                            torch.from_numpy(arg).to(DEV), torch.from_numpy(matrix).to(DEV), rc.FILL).cpu().numpy()
    _same(got, rc.layer_ref(bank[perm], op, arg, matrix), [str(i) for i in perm])


def test_layer_refuses_in_place_and_bad_shapes():
    from ssl4gie_amd import ops
    img = torch.zeros(1, 16, 16, 3, dtype=torch.uint8, device=DEV)
    op = torch.zeros(1, dtype=torch.uint8, device=DEV)
    arg = torch.zeros(1, device=DEV)
    m = torch.zeros(1, 6, dtype=torch.float64, device=DEV)
    with pytest.raises(ValueError):
        ops.randaug_layer(img, op, arg, m, rc.FILL, out=img)
    with pytest.raises(ValueError):
        ops.randaug_layer(torch.zeros(1, 18, 18, 3, dtype=torch.uint8, device=DEV), op, arg, m, rc.FILL)
    with pytest.raises(ValueError):
        ops.randaug_layer(img, op, arg, m.float(), rc.FILL)


def test_quantize_is_bit_equal():
    from ssl4gie_amd import ops
    rs = np.random.RandomState(0)
    x = (rs.rand(3, 3, 20, 20) * 280.0 - 12.0).astype(np.float32)            # below 0 and above 255 included
    x[0, 0, 0, :14] = [-3.0, -0.0, 0.0, 0.49999997, 0.5, 1.5, 2.5, 254.4, 254.5, 255.0, 255.5, 300.0, np.nan, np.inf]
    x[1] = np.floor(x[1]) + 0.5                                               # values at .5
    got = ops.quantize_u8(torch.from_numpy(x).to(DEV))
    assert got.dtype == torch.uint8 and tuple(got.shape) == (3, 20, 20, 3)
    assert np.array_equal(got.cpu().numpy(), rc.quantize_ref(x))


# ---------------------------------------------------------------------------------------------- normalize + erase
ERASE_S = 20
ERASE_BOXES = np.array([[0, 3, 5, 9], [4, 0, 7, 6], [13, 2, 7, 11], [6, 12, 5, 8],     # touching top, left, bottom, right
                        [0, 0, 0, 0], [5, 5, 0, 7], [0, 0, 19, 19], [3, 4, 1, 1],       # empty twice, nearly all, one pixel
                        [2, 2, 6, 6], [15, 2, 6, 6], [2, 2, 6, 6]], dtype=np.int32)     # [9] is not inside the image
BAD = 9


@pytest.fixture(scope="module")
def erase_case():
    from ssl4gie_amd import ops
    imgs = np.stack([rc.image(ERASE_S, i) for i in range(len(ERASE_BOXES))])
    dev = torch.from_numpy(imgs).to(DEV)
    plain = ops.normalize_u8(dev, rc.IMAGENET_MEAN, rc.IMAGENET_STD).cpu().numpy()
    return dev, plain, rc.box_mask(ERASE_BOXES, ERASE_S)


def _erase(dev, mode, seed, boxes=ERASE_BOXES):
    from ssl4gie_amd import ops
    return ops.normalize_erase_u8(dev, torch.from_numpy(boxes).to(DEV), mode, seed, rc.IMAGENET_MEAN,
                                  rc.IMAGENET_STD).cpu().numpy()


@pytest.mark.parametrize("mode", ["const", "rand", "pixel"])
def test_normalize_erase_outside_the_box_and_the_bad_box(mode, erase_case):
    dev, plain, inside = erase_case
    got = _erase(dev, mode, 5)
    assert got.dtype == np.float32 and got.shape == plain.shape
    assert np.isnan(got[BAD]).all()                    # the header: a box not inside the image -> an all-NaN sample
    keep = np.ones(len(ERASE_BOXES), dtype=bool)
    keep[BAD] = False
    outside = np.broadcast_to(~inside, got.shape)
    assert np.array_equal(got[keep][outside[keep]].view(np.uint32), plain[keep][outside[keep]].view(np.uint32))
    assert np.isfinite(got[keep]).all()
    assert np.array_equal(got[4].view(np.uint32), plain[4].view(np.uint32))      # empty boxes: nothing erased
    assert np.array_equal(got[5].view(np.uint32), plain[5].view(np.uint32))
    ins = np.broadcast_to(inside, got.shape)
    if mode == "const":
        assert (got[keep][ins[keep]].view(np.uint32) == 0).all()                 # +0.0 exactly
    if mode == "rand":
        z64 = rc.noise_field(5, len(ERASE_BOXES), ERASE_S, np.float64, rand_mode=True)
        for b in np.nonzero(keep)[0]:
            for c in range(3):
                v = got[b, c][inside[b, 0]]
                assert v.size == 0 or (v.view(np.uint32) == v.view(np.uint32)[0]).all()
                assert v.size == 0 or abs(float(v[0]) - z64[b, c, 0, 0]) < 1e-5


def test_normalize_erase_pixel_noise_against_fp64(erase_case):
    dev, _, inside = erase_case
    seed = 0x1234567890abcdef
    got = _erase(dev, "pixel", seed)
    B = len(ERASE_BOXES)
    z64 = rc.noise_field(seed, B, ERASE_S, np.float64)
    z32 = rc.noise_field(seed, B, ERASE_S, np.float32)
    sel = np.broadcast_to(inside, got.shape).copy()
    sel[BAD] = False
    err32 = float(np.abs(z32.astype(np.float64) - z64)[sel].max())
    err = float(np.abs(got.astype(np.float64) - z64)[sel].max())
    print(f"normalize_erase_u8 pixel noise: {int(sel.sum())} values, max |kernel - fp64| = {err:.3e}, float32 CPU "
          f"evaluation {err32:.3e}, bar {4 * err32:.3e}")
    valid = np.delete(ERASE_BOXES, BAD, axis=0)
    assert sel.sum() == 3 * int((valid[:, 2] * valid[:, 3]).sum()) > 1500
    assert err <= 4.0 * err32, (err, 4.0 * err32)
    # the same seed gives the same bits; another seed does not; a different B gives the shared samples the same values
    again = _erase(dev, "pixel", seed)
    assert np.array_equal(got.view(np.uint32), again.view(np.uint32))
    other = _erase(dev, "pixel", seed + 1)
    assert not np.array_equal(other[0], got[0])
    fewer = _erase(dev[:3].contiguous(), "pixel", seed, ERASE_BOXES[:3])
    assert np.array_equal(fewer.view(np.uint32), got[:3].view(np.uint32))


def test_random_erasing_class_erases_the_boxes_it_draws():
    from ssl4gie_amd import ops
    from ssl4gie_amd.data import RandomErasing
    S, B = 16, 12
    dev = torch.from_numpy(np.stack([rc.image(S, i) for i in range(B)])).to(DEV)
    g = torch.Generator(device=DEV).manual_seed(2)
    box = RandomErasing(0.5, "const", generator=_clone(g)).draw(B, S, S, DEV).cpu().numpy()
    got = RandomErasing(0.5, "const", generator=g)(dev, 0).cpu().numpy()
    inside = np.broadcast_to(rc.box_mask(box, S), got.shape)
    erased = (box[:, 2] > 0).sum()
    assert 0 < erased < B and (box[:, 0] + box[:, 2] <= S).all() and (box[:, 1] + box[:, 3] <= S).all()
    assert (got[inside] == 0).all()
    assert np.array_equal(got[~inside].view(np.uint32), ops.normalize_u8(dev).cpu().numpy()[~inside].view(np.uint32))


# ---------------------------------------------------------------------------------------------- the transform
def _bank(n, Hs, Ws):
    from ssl4gie_amd.data import DeviceImageBank
    rs = np.random.RandomState(4)
    y, x = np.mgrid[0:Hs, 0:Ws]
    imgs = np.stack([np.clip(np.stack([128 + 100 * np.sin(0.2 * x + i + c) * np.cos(0.15 * y - c) for c in range(3)], axis=2)
                             + rs.randint(-20, 20, size=(Hs, Ws, 3)), 0, 255).astype(np.uint8) for i in range(n)])
    return DeviceImageBank.from_uint8(imgs, DEV, labels=np.arange(n) % 5), imgs


def test_mae_finetune_transform_through_the_loader_is_the_staged_restatement():
    from ssl4gie_amd import ops
    from ssl4gie_amd.data import DeviceLoader, MAEFinetuneTransform
    S, B = 32, 8
    bank, _ = _bank(B, 40, 48)
    g = torch.Generator(device=DEV).manual_seed(7)
    t = MAEFinetuneTransform(S, re_prob=0.6, generator=g, noise_seed=11)
    replay = MAEFinetuneTransform(S, re_prob=0.6, generator=_clone(g), noise_seed=11)
    loader = DeviceLoader(bank, B, sampler=torch.utils.data.SequentialSampler(bank), transform=t)
    (out, labels), = list(loader)
    assert out.dtype == torch.float32 and tuple(out.shape) == (B, 3, S, S) and out.is_cuda
    assert labels.dtype == torch.int64 and labels.tolist() == [i % 5 for i in range(B)]

    index = torch.arange(B, device=DEV)
    box, flip, layers, ebox, seed = replay.draw(B, 40, 48, DEV)
    assert seed == 11 and tuple(layers[0].shape) == (2, B)
    x = ops.view_sample_u8(bank.images, index, box, flip, S, "bicubic", (0.0, 0.0, 0.0), (1.0 / 255.0,) * 3)
    u8 = rc.quantize_ref(x.cpu().numpy())
    for op, arg, matrix in zip(*layers):
        u8 = rc.layer_ref(u8, op.cpu().numpy(), arg.cpu().numpy(), matrix.cpu().numpy())
    plain = ops.normalize_u8(torch.from_numpy(u8).to(DEV), rc.IMAGENET_MEAN, rc.IMAGENET_STD).cpu().numpy()
    inside = np.broadcast_to(rc.box_mask(ebox.cpu().numpy(), S), plain.shape)
    got = out.cpu().numpy()
    assert 0 < inside.sum() < inside.size and (layers[0].cpu().numpy() != rc.SKIP).any()
    assert np.array_equal(got[~inside].view(np.uint32), plain[~inside].view(np.uint32))
    z64, z32 = rc.noise_field(seed, B, S, np.float64), rc.noise_field(seed, B, S, np.float32)
    err32 = float(np.abs(z32 - z64)[inside].max())
    err = float(np.abs(got - z64)[inside].max())
    print(f"MAEFinetuneTransform: erased share {inside.mean():.3f}, noise max |kernel - fp64| = {err:.3e}, float32 CPU "
          f"evaluation {err32:.3e}, bar {4 * err32:.3e}")
    assert err <= 4.0 * err32
    # the second call takes the next noise seed and fresh draws
    out2 = t(bank, index)
    assert t.calls == 2 and not torch.equal(out2, out)


def test_mae_finetune_transform_without_augmentation_is_crop_quantise_normalise():
    from ssl4gie_amd import ops
    from ssl4gie_amd.data import DeviceLoader, MAEFinetuneTransform, RandomResizedCropFlip
    S, B = 32, 4
    bank, _ = _bank(B, 40, 48)
    g = torch.Generator(device=DEV).manual_seed(3)
    crop = RandomResizedCropFlip(S, scale=(0.08, 1.0), mean=(0.0, 0.0, 0.0), std=(1.0 / 255.0,) * 3, generator=_clone(g))
    t = MAEFinetuneTransform(S, auto_augment=None, re_prob=0.0, generator=g)
    loader = DeviceLoader(bank, B, sampler=torch.utils.data.SequentialSampler(bank), transform=t)
    (out, _), = list(loader)
    want = ops.normalize_u8(ops.quantize_u8(crop(bank, torch.arange(B, device=DEV))))
    assert torch.equal(out.view(torch.int32), want.view(torch.int32))


def test_mae_finetune_eval_transform_is_the_centre_slice_bit_for_bit():
    from ssl4gie_amd import ops
    from ssl4gie_amd.data import DeviceLoader, MAEFinetuneTransform
    S = 28
    t = MAEFinetuneTransform.eval(S)
    M, off = t.stored, t.offset
    assert (M, off) == (32, 2)
    bank, imgs = _bank(5, M, M)
    loader = DeviceLoader(bank, 5, sampler=torch.utils.data.SequentialSampler(bank), transform=t)
    (out, _), = list(loader)
    want = ops.normalize_u8(torch.from_numpy(np.ascontiguousarray(imgs[:, off:off + S, off:off + S])).to(DEV))
    assert torch.equal(out.view(torch.int32), want.view(torch.int32))
    other, _ = _bank(2, 40, 40)
    with pytest.raises(ValueError, match="32"):
        t(other, torch.arange(2, device=DEV))
