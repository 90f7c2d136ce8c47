"""CPU: the restatement of the colour-augmentation rule (tests/colour_checks.py) against PIL, one op at a time, on
the fixed uint8 images; figures in 0..255 levels.  PIL works on 8-bit images and the rule does not round between
ops, so these are not parity bars:
  brightness, contrast, saturation  <= 1.5 levels: PIL quantises the degenerate image (the rounded mean, the "L"
                                    image) and truncates the blend
  grayscale                         <= 0.51: PIL rounds "L"
  solarize                          exact after rounding to levels
  hue, blur                         regression ALARMS at 1.25 x what the restatement gave when it was written (PIL
                                    keeps H in 8 bits and truncates the shift to int(f 255): 12.0 levels; PIL's
                                    GaussianBlur is a three-pass box approximation: 10.0 levels over the whole image
                                    at sigma = 2, 2.8 levels 8 pixels inside it)."""
import numpy as np
import pytest
import torch

import colour_checks as cc

S = 32


def _ref_levels(op=None, f=0.0, flags=0, sigma=0.0):
    """the five fixed images through ONE op of the rule -> float64 [5, S, S, 3] in levels"""
    x = cc.fixed_images(S)
    B = x.shape[0]
    factors = torch.tensor([[1.0, 1.0, 1.0, 0.0]] * B, dtype=torch.float32)
    order = torch.full((B, 4), cc.SKIP, dtype=torch.uint8)
    if op is not None:
        factors[:, op] = f
        order[:, 0] = op
    out, _ = cc.color_ref(x, factors, order, torch.full((B,), flags, dtype=torch.uint8),
                          torch.full((B,), sigma, dtype=torch.float32))
    return out.permute(0, 2, 3, 1).numpy() * 255.0


def _pil_levels(fn):
    from PIL import Image
    u8 = cc.fixed_images_u8(S)
    return np.stack([np.asarray(fn(Image.fromarray(u8[k])).convert("RGB")).astype(np.float64) for k in range(len(u8))])


@pytest.mark.parametrize("name,op,factors", [("Brightness", 0, (0.6, 1.4)), ("Contrast", 1, (0.6, 1.4)),
                                             ("Color", 2, (0.8, 1.2))])
def test_blend_ops_against_pil_imageenhance(name, op, factors):
    from PIL import ImageEnhance
    for f in factors:
        err = float(np.abs(_ref_levels(op, f) - _pil_levels(lambda im: getattr(ImageEnhance, name)(im).enhance(f))).max())
        print(f"{name} f={f}: max |restatement - PIL| = {err:.3f} levels (gate 1.5)")
        assert err <= 1.5, (name, f, err)


def test_grayscale_and_solarize_against_pil():
    from PIL import ImageOps
    err = float(np.abs(_ref_levels(flags=1) - _pil_levels(lambda im: im.convert("L"))).max())
    print(f"grayscale: {err:.4f} levels (gate 0.51)")
    assert err <= 0.51, err
    assert np.array_equal(np.rint(_ref_levels(flags=2)), _pil_levels(lambda im: ImageOps.solarize(im, 128)))


def _pil_hue(im, f):
    """torchvision's PIL adjust_hue: H of the 8-bit HSV image shifted by int(f 255), wrapping"""
    from PIL import Image
    h, s, v = im.convert("HSV").split()
    nh = ((np.asarray(h).astype(np.int64) + int(f * 255)) % 256).astype(np.uint8)
    return Image.merge("HSV", (Image.fromarray(nh, "L"), s, v)).convert("RGB")


def test_hue_against_pil_alarm():
    worst = 0.0
    for f in (-0.1, 0.1):
        d = np.abs(_ref_levels(3, f) - _pil_levels(lambda im: _pil_hue(im, f))).max(axis=(1, 2, 3))
        print(f"hue f={f}: per image {np.round(d, 2)} levels")
        assert d[2] <= 1e-3 and d[3] == 0.0 and d[4] <= 1e-3          # gray, black, white keep their values
        worst = max(worst, float(d.max()))
    print(f"hue: {worst:.2f} levels (alarm at 1.25 x 12.0)")
    assert worst <= 1.25 * 12.0, worst


def test_blur_against_pil_alarm():
    from PIL import ImageFilter
    whole = inner = 0.0
    for sigma in (1.0, 2.0):
        d = np.abs(_ref_levels(sigma=sigma) - _pil_levels(lambda im: im.filter(ImageFilter.GaussianBlur(radius=sigma))))
        print(f"blur sigma={sigma}: whole {d.max():.2f}, 8 pixels in {d[:, 8:-8, 8:-8].max():.2f} levels")
        assert d[3].max() == 0.0 and d[4].max() <= 1e-3               # black and white stay what they are
        whole, inner = max(whole, float(d.max())), max(inner, float(d[0, 8:-8, 8:-8].max()))
    print(f"blur: whole image {whole:.2f} (alarm at 1.25 x 10.0), interior on noise {inner:.2f} (alarm at 1.25 x 2.8)")
    assert whole <= 1.25 * 10.0 and inner <= 1.25 * 2.8, (whole, inner)


def test_restatement_basics():
    x = cc.fixed_images(S)
    B = x.shape[0]
    ident = torch.tensor([[1.0, 1.0, 1.0, 0.0]] * B, dtype=torch.float32)
    skip = torch.full((B, 4), cc.SKIP, dtype=torch.uint8)
    zero_u8, zero_f = torch.zeros(B, dtype=torch.uint8), torch.zeros(B, dtype=torch.float32)
    # all skipped: clamp(x, 0, 1), in float32 bit for bit
    out, pre = cc.color_ref(x * 1.5 - 0.2, ident, skip, zero_u8, zero_f, dtype=torch.float32)
    assert torch.equal(out, (x * 1.5 - 0.2).clamp(0, 1)) and torch.equal(out, pre)
    # an op id above 3 is a skip, whatever its value
    odd = skip.clone()
    odd[:, 1] = 7
    assert torch.equal(cc.color_ref(x, ident, odd, zero_u8, zero_f)[0], cc.color_ref(x, ident, skip, zero_u8, zero_f)[0])
    # identity factors with a real order change nothing (hue by 0 is a round trip through hsv)
    real = torch.tensor([[3, 1, 0, 2]] * B, dtype=torch.uint8)
    assert float((cc.color_ref(x, ident, real, zero_u8, zero_f)[0] - x.double()).abs().max()) <= 1e-12
    # hue by a whole turn is the identity too, and the gray image keeps its value under any shift
    turn = ident.clone()
    turn[:, 3] = 0.25
    h = torch.tensor([[3, 255, 255, 255]] * B, dtype=torch.uint8)
    v = x.double()
    for _ in range(4):
        v = cc.color_ref(v, turn, h, zero_u8, zero_f)[0]
    assert float((v - x.double()).abs().max()) <= 1e-12
    assert torch.equal(cc.color_ref(x, turn, h, zero_u8, zero_f)[0][2], x[2].double())
    # contrast uses the mean of the CURRENT image: brightness first changes it
    bc = torch.tensor([[0.5, 1.5, 1.0, 0.0]] * B, dtype=torch.float32)     # exact in float32
    a = cc.color_ref(x, bc, torch.tensor([[0, 1, 255, 255]] * B, dtype=torch.uint8), zero_u8, zero_f)[0]
    m = cc.gray(x.double() * 0.5).mean(dim=(1, 2, 3), keepdim=True)
    assert float((a - (1.5 * 0.5 * x.double() - 0.5 * m).clamp(0, 1)).abs().max()) <= 1e-12
    # normalise
    n = cc.color_ref(x, ident, skip, zero_u8, zero_f, (0.485, 0.456, 0.406), (0.229, 0.224, 0.225))[0]
    want = (x.double() - torch.tensor((0.485, 0.456, 0.406), dtype=torch.float64).view(1, 3, 1, 1)) \
        / torch.tensor((0.229, 0.224, 0.225), dtype=torch.float64).view(1, 3, 1, 1)
    assert float((n - want).abs().max()) <= 1e-12


def test_restatement_blur_pieces():
    assert [cc.radius(torch.tensor(s, dtype=torch.float32)) for s in cc.SIGMAS[1:]] == [1, 2, 3, 6]
    assert cc.radius(torch.tensor(1.0 / 3.0, dtype=torch.float32)) == 2      # float32(1/3) is above 1/3
    assert cc.radius(torch.tensor(50.0, dtype=torch.float32)) == 6
    assert cc.symmetric_index(8, 6).tolist() == [5, 4, 3, 2, 1, 0, 0, 1, 2, 3, 4, 5, 6, 7, 7, 6, 5, 4, 3, 2]
    for sigma in cc.SIGMAS[1:]:
        R = cc.radius(torch.tensor(sigma, dtype=torch.float32))
        w = cc.gaussian_weights(torch.tensor(sigma, dtype=torch.float64), R, torch.float64)
        assert len(w) == 2 * R + 1 and abs(float(w.sum()) - 1.0) <= 1e-15 and torch.equal(w, w.flip(0))
        assert abs(float(w[R + 1] / w[R]) - np.exp(-0.5 / sigma ** 2)) <= 1e-15
        flat = torch.full((3, 8, 8), 0.37, dtype=torch.float64)
        assert float((cc.blur(flat, torch.tensor(sigma, dtype=torch.float64), R) - 0.37).abs().max()) <= 1e-15
    # an impulse away from the edges spreads as the outer product of the weights; one at the corner folds back
    imp = torch.zeros(3, 24, 24, dtype=torch.float64)
    imp[:, 12, 11] = 1.0
    w = cc.gaussian_weights(torch.tensor(1.0, dtype=torch.float64), 3, torch.float64)
    got = cc.blur(imp, torch.tensor(1.0, dtype=torch.float64), 3)
    assert float((got[0, 9:16, 8:15] - torch.outer(w, w)).abs().max()) <= 1e-15 and abs(float(got[0].sum()) - 1.0) <= 1e-14
    imp = torch.zeros(3, 24, 24, dtype=torch.float64)
    imp[:, 0, 0] = 1.0
    got = cc.blur(imp, torch.tensor(1.0, dtype=torch.float64), 3)
    assert abs(float(got[0, 0, 0]) - float((w[3] + w[4]) ** 2)) <= 1e-15 and abs(float(got[0].sum()) - 1.0) <= 1e-14


def test_fixed_cases_cover_what_they_claim_and_stay_under_the_solarize_cap():
    for S_ in (24, 32):
        (x, factors, order, flags, sigma), ref64, mask, share, err32 = cc.parity_case(S_)
        assert x.shape == (30, 3, S_, S_) and x.dtype == torch.float32
        assert sorted(tuple(r) for r in order[:24].tolist()) == sorted(cc.PERMS)
        assert order[24].tolist() == [cc.SKIP] * 4 and factors[25].tolist() == [1.0, 1.0, 1.0, 0.0]
        assert set(flags.tolist()) == {0, 1, 2, 3}
        assert sorted(set(round(float(s), 2) for s in sigma)) == [0.0, 0.1, 0.34, 1.0, 2.0]
        assert {(i % 5, round(float(sigma[i]), 2)) for i in range(30)} >= {(k, 2.0) for k in range(5)}
        print(f"S={S_}: float32 evaluation error {err32:.3e}, excluded share {share:.2e}")
        assert share <= cc.SOLARIZE_EXCLUDED_MAX and 0.0 < err32 <= 1e-5
        assert bool(torch.isfinite(ref64).all())
