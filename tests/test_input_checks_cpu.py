"""CPU: the fp64 restatement of the view sampler's resampling rule (tests/input_checks.py) against torch's own
CPU F.interpolate(antialias=True) on the fixed cases — the restatement is the reference of the GPU tests."""
import numpy as np

import input_checks as ic

# torch's fp32 path sits within 3.0e-4 (bicubic) / 2.5e-4 (bilinear) of the restatement in 0..255 units on an
# 80-wide image; other torch builds order the sums differently, hence the 3x margin
GATE = 1e-3


def test_restatement_matches_torch_cpu_antialiased_interpolate():
    err = ic.torch_cpu_error()
    print("torch CPU fp32 vs fp64 restatement, 0..255 units:", err)
    assert set(err) == set(ic.FILTERS)
    for name, e in err.items():
        assert 0.0 < e < GATE, (name, e)


def test_cases_cover_tap_counts_overshoot_and_both_scalings():
    img = ic.noise_image(0)
    assert img.shape == (ic.H_IMG, ic.W_IMG, 3) and (3 * ic.W_IMG) % 4 != 0
    counts = np.concatenate([ic.tap_counts(L, S, name) for name in ic.FILTERS for S in ic.SIZES
                             for box in ic.BOXES for L in box[2:]])
    assert counts.min() == 1 and counts.max() >= 15            # 1x1 box ... 90 -> 24 and 96 -> 24 bicubic
    raw = np.concatenate([ic.resample(img, box, S, "bicubic").ravel() for box in ic.BOXES for S in ic.SIZES])
    assert raw.min() < 0.0 and raw.max() > 255.0                # bicubic overshoots: the clamp is exercised
    ref = ic.view_ref(img, ic.BOXES[0], 32, "bicubic")
    assert ref.min() >= 0.0 and ref.max() <= 255.0
    scales = [L / S for S in ic.SIZES for box in ic.BOXES for L in box[2:]]
    assert min(scales) < 1.0 < max(scales)                      # up- and down-sampling
    for L, S, name in ((96, 24, "bicubic"), (7, 32, "bilinear"), (1, 24, "bicubic")):
        np.testing.assert_allclose(ic.axis_weights(L, S, name).sum(axis=1), 1.0, rtol=0, atol=1e-14)


def test_flip_and_normalise_conventions():
    img = ic.noise_image(0)
    box = ic.BOXES[4]
    a = ic.view_ref(img, box, 24, "bilinear", flip=False)
    b = ic.view_ref(img, box, 24, "bilinear", flip=True)
    assert np.array_equal(b, a[:, :, ::-1])
    mean, std = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
    n = ic.view_ref(img, box, 24, "bilinear", mean=mean, std=std)
    for c in range(3):
        np.testing.assert_allclose(n[c], (a[c] / 255.0 - mean[c]) / std[c], rtol=0, atol=1e-12)
    # a box resampled to its own size is the identity: one tap of weight 1 per output
    same = ic.view_ref(img, (0, 0, 32, 32), 32, "bicubic")
    np.testing.assert_allclose(same, img[:32, :32].transpose(2, 0, 1), rtol=0, atol=1e-12)
