"""Proof that the BatchNorm checks of tests/bn_checks.py bite (no GPU): the plain fp32 torch evaluation of the
textbook formulae passes every check, and each deliberately wrong variant of it fails at least one — at a
mid-size map and at the largest one this test can afford (12 544 x 256, the last ResNet stage of a 256-image view).

What the real-valued checks cannot see: one row missing from (or counted twice in) the sums of a 3.2 M-row map
changes sum g by |g_r| ~ 1 against a bound of k 2^-24 sum_r |g| ~ 2.4; the exact-integer family of
tests/test_gpu_batchnorm_kernels.py (every sum an integer below 2^24, compared bit for bit) is what catches it
there, at every size.  Likewise the unbiased / biased slips are relative errors of 1 / n and fall below
k 2^-24 from n ~ 10^6; they are pinned at the sizes below and by the integer statistics tests."""
import pytest
import torch

import bn_checks as bc

F32, BF = torch.float32, torch.bfloat16
MID, LARGE = (1531, 64), (12544, 256)
# the check(s) each wrong variant must trip (any of them)
EXPECT = {
    "drop_row": {"mean", "var", "sums[0]", "sums[1]", "dbeta", "dgamma"},
    "dup_row": {"mean", "var", "sums[0]", "sums[1]", "dbeta", "dgamma"},
    "unbiased_norm": {"rstd"},
    "mask_shift": {"dres"},
    "mask_ge": {"dres", "dbeta"},
    "dres_unmasked": {"dres"},
    "sum_x_not_xhat": {"sums[1]", "dgamma"},
    "run_var_biased": {"run_var"},
    "last_strip": {"y", "dx", "dres"},
    "gamma_ignored": {"y", "dx"},
}


def case(shape, dtype, with_res=True, seed=5):
    return bc.make_case(shape[0], shape[1], dtype, "cpu", seed, True, with_res, True)


@pytest.mark.parametrize("pivot", [True, False], ids=["pivot", "about0"])
@pytest.mark.parametrize("dtype", [F32, BF], ids=["fp32", "bf16"])
@pytest.mark.parametrize("shape", [MID, LARGE], ids=["mid", "large"])
def test_fp32_evaluation_passes_every_check(shape, dtype, pivot):
    """... with a factor 4 to spare: k = max(16, 4 k_ref)"""
    for with_res in (True, False):
        c = case(shape, dtype, with_res)
        rep = bc.check_all(c, bc.fp32_eval(c, pivot), pivot)
        print(shape, dtype, pivot, with_res, {n: round(v, 4) for n, v in rep.worst.items()})
        rep.assert_ok()
        for n, v in rep.worst.items():
            if n != "tie_share":
                assert v <= bc.K[n.split("[")[0]] / 4, (n, v)
        assert rep.worst["tie_share"] <= bc.MAX_TIE_SHARE


def test_k_is_derived_from_k_ref():
    assert set(bc.K) == set(bc.CHECKS) == set(bc.K_REF)
    for n in bc.CHECKS:
        k = bc.K[n]
        assert k >= 16 and k >= 4 * bc.K_REF[n] and k & (k - 1) == 0 and (k == 16 or k < 8 * bc.K_REF[n])


@pytest.mark.parametrize("mut", bc.MUTATIONS)
@pytest.mark.parametrize("dtype,shape", [(F32, MID), (BF, MID), (F32, LARGE)], ids=["fp32-mid", "bf16-mid", "fp32-large"])
def test_wrong_variant_is_caught(mut, dtype, shape):
    c = case(shape, dtype, with_res=mut != "mask_ge")   # mask_ge: channel 1 (gamma = beta = 0) is y == 0 exactly
    if mut == "mask_ge":
        assert bool((bc.fp32_eval(c)["y"][:, 1] == 0).all())
    rep = bc.check_all(c, bc.fp32_eval(c, True, mut), True)
    assert set(rep.names()) & EXPECT[mut], (mut, rep.failed)


def test_wrong_variant_is_caught_without_relu_and_affine():
    """the sums / strip / variance slips on the affine-free, ReLU-free form (the BatchNorm that ends the MoCo heads)"""
    c = bc.make_case(256, 256, F32, "cpu", 9, False, False, False)
    bc.check_all(c, bc.fp32_eval(c)).assert_ok()
    for mut in ("drop_row", "dup_row", "unbiased_norm", "sum_x_not_xhat", "run_var_biased", "last_strip"):
        rep = bc.check_all(c, bc.fp32_eval(c, True, mut))
        assert set(rep.names()) & EXPECT[mut], (mut, rep.failed)


def test_rows_1_convention():
    """one row: variance 0, y = beta (+ res), and the running variance blended with the biased value"""
    c = bc.make_case(1, 64, F32, "cpu", 3, False, False, True)
    o = bc.fp32_eval(c)
    bc.check_all(c, o).assert_ok()
    assert torch.equal(o["var"], torch.zeros(64))
    assert torch.allclose(o["run_var"], 0.9 * c["rv0"])


def test_edge_cases_keep_the_relu_ties_within_the_cap():
    """the small edge cases of the GPU module are generated on the CPU (bn_checks.edge_case): each leaves out at
    most MAX_TIE_SHARE of its elements, at twice the exclusion radius (room for the kernels' own statistics)"""
    k2 = {n: 2 * v for n, v in bc.K.items()}
    for C in bc.EDGE_C:
        for dtype in (F32, BF):
            for rows in bc.edge_rows(C, dtype)[1:]:      # rows = 1 runs without ReLU
                for with_res in (False, True):
                    c = bc.edge_case(rows, C, dtype, True, with_res, True)
                    o = bc.fp32_eval(c)
                    rep = bc.Report(k2)
                    bc.check_forward(rep, c["x"], o["mean"], o["rstd"], c["gamma"], c["beta"], c["res"], True, o["y"])
                    assert rep.worst["tie_share"] <= bc.MAX_TIE_SHARE, (rows, C, dtype, with_res, rep.worst)
                    assert not rep.failed, rep.failed
