"""CPU: the restatement of the detection input rule (tests/det_input_checks.py) against the reference's own dataset
class (tests/golden/g21_det_loader.npz), torch's F.interpolate and warp_checks' square colour stage."""
import os

import numpy as np
import pytest
import torch

import colour_checks as cc
import det_input_checks as dc
import warp_checks as wc

G21 = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g21_det_loader.npz")


def bits(t):
    return np.ascontiguousarray(np.asarray(t, dtype=np.float32)).view(np.uint32)


def test_fixture_covers_the_issue_cases():
    cases, F = dc.g21(G21)
    assert F == 64 and os.path.getsize(G21) < 1 << 20
    shapes = [c[0].shape[:2] for c in cases]
    assert {(40, 56), (64, 64), (71, 93), (100, 50), (65, 20), (128, 128), (13, 13)} == set(shapes)
    assert {c[2] for c in cases if c[0].shape[:2] == (71, 93)} == {(r, h, v) for r in (0, 1) for h in (0, 1) for v in (0, 1)}
    assert {len(c[1]) for c in cases} == {0, 1, 3}
    halved = {c[0].shape[:2] for c in cases if dc.is_halved(c[0], c[2], F)}
    assert halved == {(71, 93), (100, 50), (65, 20), (128, 128)}


def test_restatement_equals_reference_bit_for_bit_without_halving():
    cases, F = dc.g21(G21)
    n = 0
    for img, boxes, dec, out_img, out_boxes in cases:
        if dc.is_halved(img, dec, F):
            continue
        n += 1
        for dtype in (torch.float32, torch.float64):
            got = dc.geometry_ref(dc.to_tensor(img, dtype), dec, F)
            assert np.array_equal(bits(got.to(torch.float32).numpy()), bits(out_img)), (img.shape, dec, dtype)
        assert np.array_equal(bits(dc.boxes_ref(boxes, img.shape[0], img.shape[1], dec, F).numpy()), bits(out_boxes))
    assert n == 3


def test_restatement_boxes_equal_reference_bit_for_bit_on_halved_cases():
    cases, F = dc.g21(G21)
    n = 0
    for img, boxes, dec, _, out_boxes in cases:
        if dc.is_halved(img, dec, F):
            n += 1
            got = dc.boxes_ref(boxes, img.shape[0], img.shape[1], dec, F).numpy()
            assert got.shape == out_boxes.shape and np.array_equal(bits(got), bits(out_boxes)), (img.shape, dec)
    assert n == 11


def test_restatement_halved_images_match_reference():
    """the fixture's halved images are torch's float32 F.interpolate: the float64 restatement is within a few float32
    ulps of them, and the pads are exact zeros"""
    cases, F = dc.g21(G21)
    for img, _, dec, out_img, _ in cases:
        if dc.is_halved(img, dec, F):
            got = dc.geometry_ref(dc.to_tensor(img, torch.float64), dec, F)
            err = float((got - torch.from_numpy(out_img).to(torch.float64)).abs().max())
            print(f"{img.shape[:2]} {dec}: |fp64 restatement - reference| = {err:.3e}")
            assert err < 2e-6   # two passes of at most 8 float32 products each on values in [-0.2, 1.2]: a few ulps of 1


@pytest.mark.parametrize("L", (12, 40, 14, 94))
def test_fp64_halving_matches_interpolate(L):
    g = torch.Generator().manual_seed(L)
    x = torch.rand(3, 1, L, generator=g, dtype=torch.float64)
    ref = torch.nn.functional.interpolate(x.unsqueeze(0), size=(1, L // 2), mode="bicubic", antialias=True,
                                          align_corners=False)[0]
    got = x @ dc.halve_matrix(L, torch.float64).T
    assert float((got - ref).abs().max()) < 1e-12
    x2 = torch.rand(3, L, 22, generator=g, dtype=torch.float64)
    ref2 = torch.nn.functional.interpolate(x2.unsqueeze(0), size=(L // 2, 11), mode="bicubic", antialias=True,
                                           align_corners=False)[0]
    assert float((dc.halve(x2) - ref2).abs().max()) < 1e-12


def test_odd_sides_get_a_zero_row_and_column():
    g = torch.Generator().manual_seed(5)
    x = torch.rand(3, 15, 21, generator=g, dtype=torch.float64)
    padded = torch.nn.functional.pad(x, (0, 1, 0, 1))
    ref = torch.nn.functional.interpolate(padded.unsqueeze(0), size=(8, 11), mode="bicubic", antialias=True,
                                          align_corners=False)[0]
    assert float((dc.halve(x) - ref).abs().max()) < 1e-12


def test_interior_weights_are_the_dyadic_constants():
    for dtype in (torch.float32, torch.float64):
        M = dc.halve_matrix(40, dtype)
        for i in range(2, 18):
            assert torch.equal(M[i, 2 * i - 3:2 * i + 5] * 256.0, torch.tensor(dc.DYADIC, dtype=dtype)), i
        # the first output keeps five taps, renormalised by their sum 239
        assert float((M[0, :5] - torch.tensor(dc.DYADIC[3:], dtype=torch.float64) / 239.0).abs().max()) < 1e-7
        assert float(M[0, 5:].abs().max()) == 0.0
        assert float((M.sum(dim=1) - 1.0).abs().max()) < 1e-6


@pytest.mark.parametrize("S", (16, 32))
def test_rectangular_colour_restatement_equals_the_square_one(S):
    x, factors, order, flags, sigma = wc.ft_rows(S)
    for dtype in (torch.float64, torch.float32):
        sq = wc.color_ft_ref(x, factors, order, flags, sigma, cc.ZERO3, cc.ONE3, dtype)
        rect = dc.color_rect_ref(x, factors, order, sigma, dtype)
        assert torch.equal(sq, rect), dtype


def test_blur_axes_are_not_swapped():
    """a vertical step edge stays constant along columns under the rectangular blur, and the other way round"""
    x = torch.zeros(3, 14, 30, dtype=torch.float64)
    x[:, :, 15:] = 1.0
    y = dc.blur25_rect(x, 1.5)
    assert float((y - y[:, :1, :]).abs().max()) < 1e-15 and float((y[:, 0, 14] - y[:, 0, 15]).abs().max()) > 0.1


def test_box_rule_by_hand():
    b = np.array([[10.0, 20.0, 30.0, 50.0]], np.float32)
    # 71 x 93, rotate: (20, 93 - 30, 50, 93 - 10) in a 93 x 71 image; halved: / 2; pads p1 = (64 - 36) // 2, p2 = (64 - 47) // 2
    got = dc.boxes_ref(b, 71, 93, (1, 0, 0), 64).tolist()
    assert got == [[10.0 + 14, 31.5 + 8, 25.0 + 14, 41.5 + 8]]
    assert dc.out_geometry(71, 93, 0, 64) == (71, 93, True, 36, 47, 8, 14)
    for dec in [(r, h, v) for r in (0, 1) for h in (0, 1) for v in (0, 1)]:
        assert dc.bits_dec(dc.geom_bits(dec)) == dec
