"""CPU: the restatements of tests/randaug_checks.py against PIL, bit for bit, over the fixed cases the GPU tests
reuse; timm's level maps, the erase boxes and the noise stream against their literal forms.  timm is not installed:
its rules are restated from timm 0.3.2's published source, PIL (present) is the arbiter of every pixel rule."""
import math

import numpy as np
import pytest
import torch

import randaug_checks as rc

Image = pytest.importorskip("PIL.Image")
from PIL import ImageEnhance, ImageOps   # noqa: E402

SIZES = (16, 20, 36, 64)


def _pil(arr):
    return Image.fromarray(arr, "RGB")


def _pil_op(img, op, arg, matrix, S):
    """the PIL call timm makes for op (auto_augment.py), resample = BICUBIC and fillcolor = FILL"""
    kw = dict(resample=Image.BICUBIC, fillcolor=rc.FILL)
    im = _pil(img)
    if op == rc.AUTO_CONTRAST:
        out = ImageOps.autocontrast(im)
    elif op == rc.EQUALIZE:
        out = ImageOps.equalize(im)
    elif op == rc.INVERT:
        out = ImageOps.invert(im)
    elif op == rc.ROTATE:
        out = im.rotate(arg, **kw)
    elif op == rc.POSTERIZE:
        out = im if int(arg) >= 8 else ImageOps.posterize(im, int(arg))
    elif op == rc.SOLARIZE:
        out = ImageOps.solarize(im, int(arg))
    elif op == rc.SOLARIZE_ADD:
        lut = [min(255, i + int(arg)) if i < 128 else i for i in range(256)]
        out = im.point(lut + lut + lut)
    elif op == rc.COLOR:
        out = ImageEnhance.Color(im).enhance(arg)
    elif op == rc.CONTRAST:
        out = ImageEnhance.Contrast(im).enhance(arg)
    elif op == rc.BRIGHTNESS:
        out = ImageEnhance.Brightness(im).enhance(arg)
    elif op == rc.SHARPNESS:
        out = ImageEnhance.Sharpness(im).enhance(arg)
    else:
        out = im.transform(im.size, Image.AFFINE, tuple(matrix), **kw)
    return np.asarray(out)


@pytest.mark.parametrize("S", SIZES)
def test_every_op_restatement_is_pil_bit_for_bit(S):
    """every case of op_cases(S).  Rotations: PIL rounds cos and sin to 15 decimals, so the restatement is given
    PIL's rounded matrix here; with the unrounded matrix of the fixed cases at most a few bytes may move, counted below"""
    moved = 0
    for i, (name, kind, op, arg, matrix) in enumerate(rc.op_cases(S)):
        img = rc.image(S, i % 7, kind)
        want = _pil_op(img, op, float(arg), matrix, S)
        m = rc.rotate_matrix(arg, S, rounded=True) if op == rc.ROTATE else matrix
        got = rc.apply_op(img, op, arg, m)
        assert got.dtype == np.uint8 and np.array_equal(got, want), (S, name, int((got != want).sum()))
        if op == rc.ROTATE:
            moved += int((rc.apply_op(img, op, arg, matrix) != want).sum())
    print(f"S={S}: bytes that differ between the unrounded and PIL's rounded rotation matrix: {moved}")
    assert moved <= 0.001 * 4 * S * S * 3


def test_pil_takes_the_branches_the_cases_are_there_for():
    h = rc.hist(rc.image(16, 0, "const_channel")[..., 1])
    assert (h > 0).sum() == 1 and rc.equalize_step(h) is None
    assert np.array_equal(rc.lut_autocontrast(h), np.arange(256))
    for c in range(3):
        assert rc.equalize_step(rc.hist(rc.image(16, 0, "step_zero")[..., c])) == 0
        h1 = rc.hist(rc.image(16, 0, "step_one")[..., c])
        assert h1[np.nonzero(h1)[0][-1]] == 1 and rc.equalize_step(h1) == 1
    img = rc.image(16, 0, "step_one")
    assert not np.array_equal(rc.apply_op(img, rc.EQUALIZE), img)       # a real table, not the identity
    assert np.array_equal(rc.apply_op(rc.image(16, 0, "step_zero"), rc.EQUALIZE), rc.image(16, 0, "step_zero"))
    hl = rc.hist(rc.lum(rc.image(20, 0, "half_mean")))
    mean = sum(i * int(hl[i]) for i in range(256)) / hl.sum()
    assert mean == 10.5 and rc.contrast_mean(hl) == 11
    # the geometric cases reach the fill colour AND interpolated pixels AND clamped taps
    img = rc.image(20, 0, "noise")
    out = rc.affine(img, rc.op_matrix(rc.TRANSLATE_X, -1.37, 20))
    fill = (out == np.array(rc.FILL, np.uint8)).all(axis=2)
    assert 0 < fill.sum() < 400


def test_nan_matrix_fills_and_skip_copies():
    img = rc.image(16, 1)
    out = rc.affine(img, (float("nan"),) * 6)
    assert (out == np.array(rc.FILL, np.uint8)).all()
    assert np.array_equal(rc.apply_op(img, rc.SKIP), img) and np.array_equal(rc.apply_op(img, 15), img)


def test_quantize_restatement():
    x = np.array([-3.0, -0.0, 0.0, 0.49999997, 0.5, 1.5, 2.5, 254.4, 254.5, 255.0, 255.5, 300.0, np.nan, np.inf],
                 dtype=np.float32)
    want = np.array([0, 0, 0, 1, 1, 2, 3, 254, 255, 255, 255, 255, 0, 255], dtype=np.uint8)
    pad = np.zeros(16 * 3 - x.size, dtype=np.float32)
    q = rc.quantize_ref(np.concatenate([x, pad]).reshape(1, 3, 4, 4))
    assert np.array_equal(q.transpose(0, 3, 1, 2).reshape(-1)[:x.size], want)


@pytest.mark.parametrize("inc", [0, 1])
@pytest.mark.parametrize("magnitude", [0.0, 9.0, 10.0, 4.37])
def test_level_maps_match_the_literal_transcription(inc, magnitude):
    from ssl4gie_amd.data import randaug_level_args
    S = 224
    for negate in (False, True):
        op = torch.arange(rc.N_OPS, dtype=torch.int64)
        mag = torch.full((rc.N_OPS,), magnitude, dtype=torch.float64)
        neg = torch.full((rc.N_OPS,), negate)
        arg, matrix = randaug_level_args(op, mag, neg, inc, S)
        assert arg.dtype == torch.float32 and matrix.dtype == torch.float64 and tuple(matrix.shape) == (rc.N_OPS, 6)
        for o in range(rc.N_OPS):
            want = rc.timm_level_arg(o, magnitude, negate, inc, S)
            if want is None:
                assert float(arg[o]) == 0.0
            else:
                assert float(arg[o]) == float(np.float32(want)), (o, float(arg[o]), want)
            m = rc.op_matrix(o, want, S) if o in rc.GEOMETRIC else rc.IDENTITY
            assert matrix[o].tolist() == pytest.approx(list(m), rel=0, abs=1e-12), (o, matrix[o].tolist(), m)
            if o != rc.ROTATE:
                assert matrix[o].tolist() == list(m)


def test_randaug_draw_shapes_skips_and_config():
    from ssl4gie_amd.data import RandAugment
    g = torch.Generator().manual_seed(5)
    ra = RandAugment("rand-m9-mstd0.5-inc1", 224, generator=g)
    assert (ra.magnitude, ra.layers, ra.mstd, ra.inc) == (9.0, 2, 0.5, 1) and ra.fill == rc.FILL
    op, arg, matrix = ra.draw(4000, "cpu")
    assert op.dtype == torch.uint8 and tuple(op.shape) == (4000, 2)
    assert arg.dtype == torch.float32 and tuple(arg.shape) == (4000, 2)
    assert matrix.dtype == torch.float64 and tuple(matrix.shape) == (4000, 2, 6)
    skipped = float((op == rc.SKIP).double().mean())
    assert abs(skipped - 0.5) < 0.03
    kept = op[op != rc.SKIP].long()
    counts = torch.bincount(kept, minlength=rc.N_OPS)
    assert int(kept.max()) == rc.N_OPS - 1 and int(counts.min()) > 0.6 * kept.numel() / rc.N_OPS
    ra3 = RandAugment("rand-m7-n3-mstd0", 32)
    assert (ra3.magnitude, ra3.layers, ra3.mstd, ra3.inc) == (7.0, 3, 0.0, 0)
    with pytest.raises(NotImplementedError):
        RandAugment("rand-m9-w0", 224)
    with pytest.raises(ValueError):
        RandAugment("augmix-m3", 224)


def test_erase_boxes_match_the_literal_loop():
    from ssl4gie_amd.data import erase_boxes
    u = np.random.RandomState(3).rand(3000, 41)
    u[:5, 0] = 0.0
    for (H, W, p, kw) in ((224, 224, 0.25, {}), (16, 16, 1.0, {}), (36, 36, 1.0, dict(max_area=1.0, min_aspect=0.1))):
        want = rc.erase_boxes_loop(u, H, W, p, **kw)
        got = erase_boxes(torch.from_numpy(u), H, W, p, **kw)
        assert got.dtype == torch.int32 and np.array_equal(got.numpy(), want)
        assert (want[:, 2] > 0).any() and ((want[:, 0] + want[:, 2]) <= H).all()
    assert (rc.erase_boxes_loop(u, 36, 36, 1.0, max_area=1.0, min_aspect=0.1)[:, 2] == 0).any()   # ten misses happen


def test_random_erasing_refuses_more_than_one_box():
    from ssl4gie_amd.data import RandomErasing
    with pytest.raises(NotImplementedError):
        RandomErasing(max_count=2)
    with pytest.raises(ValueError):
        RandomErasing(mode="other")


def test_philox_known_answers():
    """Random123's kat_vectors for philox4x32-10"""
    z = np.zeros(1, np.uint64)
    assert [int(w[0]) for w in rc.philox4x32_10(z, z, z, z, 0, 0)] == [0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8]
    f = z + np.uint64(0xffffffff)
    assert [int(w[0]) for w in rc.philox4x32_10(f, f, f, f, 0xffffffff, 0xffffffff)] == \
        [0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd]
    c = [z + np.uint64(v) for v in (0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344)]
    assert [int(w[0]) for w in rc.philox4x32_10(*c, 0xa4093822, 0x299f31d0)] == \
        [0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1]


def test_noise_is_standard_normal():
    """seed 2024, 2 x 3 x 96 x 96 = 55 296 values: mean, variance and the Kolmogorov-Smirnov distance to Phi below the
    1 % critical value 1.63 / sqrt(n).  Deterministic: this seed passes"""
    z = rc.noise_field(2024, 2, 96, np.float64).reshape(-1)
    n = z.size
    assert n >= 50000
    assert abs(z.mean()) < 4.0 / math.sqrt(n) and abs(z.var() - 1.0) < 4.0 * math.sqrt(2.0 / n)
    zs = np.sort(z)
    cdf = np.array([0.5 * (1.0 + math.erf(v / math.sqrt(2.0))) for v in zs])
    i = np.arange(1, n + 1)
    d = max(np.max(i / n - cdf), np.max(cdf - (i - 1) / n))
    print(f"noise: n = {n}, mean {z.mean():.4e}, var {z.var():.5f}, KS distance {d:.5f}, bar {1.63 / math.sqrt(n):.5f}")
    assert d < 1.63 / math.sqrt(n)
    z32 = rc.noise_field(2024, 2, 96, np.float32).reshape(-1)
    assert z32.dtype == np.float32 and np.abs(z32 - z).max() < 1e-5
    r = rc.noise_field(2024, 2, 96, np.float64, rand_mode=True)
    assert r.shape == (2, 3, 1, 1) and np.array_equal(r[:, :, 0, 0], rc.noise_field(2024, 2, 4, np.float64)[:, :, 0, 0])


def test_eval_transform_box_and_refusal():
    from ssl4gie_amd.data import MAEFinetuneTransform
    t = MAEFinetuneTransform.eval(224)
    assert t.stored == 256 and t.offset == 16
    assert MAEFinetuneTransform.eval(384).stored == 384
    assert MAEFinetuneTransform.eval(32).stored == int(32 / (224 / 256)) and MAEFinetuneTransform.eval(32).offset == 2

    class Bank:
        stored_size = (224, 224)
    with pytest.raises(ValueError, match="256"):
        t(Bank(), torch.zeros(1, dtype=torch.int64))
