"""Proof that the attention checks of tests/attn_checks.py bite (no GPU): the plain fp32 torch emulation of the
kernels' interface (P and dS rounded to bf16 once, fp32 sums, bf16 outputs; either normaliser convention) passes
every check in every case family, and each deliberately wrong variant of it fails the check named in EXPECT, in the
family named there.

The gap this closes.  One zero-padded key that joins the softmax (`pad_leak`: what the `kt >= NKT - 2` masking, the
HT variants and the MASK variants of csrc/attention.hip exist to prevent) is NOT caught by random operands at the
sizes a network has: at N = 197, hd 32, `gauss` at scale 1.5 or 3 the leak moves O by a fraction of the bf16 rounding
error and lse by less than the 2^-8 the sum of rounded probabilities is worth
(test_padded_key_leak_is_invisible_to_gauss_at_hd32 states it).  In the `uniform` family every probability is
exactly representable, lse is pinned at the 2^-24 level, and the leak is a 1 / (N + 1) error there: it is caught at
EVERY N from 1 to 256 (test_padded_key_leak_is_caught_at_every_n)."""
import pytest
import torch

import attn_checks as ac

F32, BF = ac.F32, ac.BF
NS = ac.ONE_PER_BUCKET + (300, 512)        # one N per whole-head bucket, a masked and an unmasked streaming N


def cases_at(N, hd, dtype, B=2, H=2):
    out = [ac.make_case("gauss", B, N, H, hd, dtype, seed=3, scale=sc, offset=off) for sc, off in ac.GAUSS_VARIANTS]
    out += [ac.make_case("uniform", B, N, H, hd, dtype, seed=3, s0=s0) for s0 in ac.UNIFORM_S0]
    if dtype == BF:       # the GPU module runs onehot on the bf16 kernels only
        out.append(ac.make_case("onehot", B, N, H, hd, dtype, seed=3))
    return out


@pytest.mark.parametrize("hd", [32, 64])
@pytest.mark.parametrize("N", NS)
def test_emulation_passes_every_check_bf16(N, hd):
    """... under either normaliser convention, with a factor 4 to spare: k = max(16, 4 k_ref)"""
    for c in cases_at(N, hd, BF):
        for norm, kernel in (("rounded", "whole32"), ("fp32", "whole64")):
            c["kernel"] = kernel
            rep = ac.check_all(c, ac.emu_eval(c, norm))
            rep.assert_ok()
            for n, v in rep.worst.items():
                assert v <= ac.K[n] / 4, (c["tag"], norm, n, v)
            for n, v in rep.worst_u.items():       # the derived c holds for the reference itself
                assert v <= 1.0, (c["tag"], norm, n, v)


@pytest.mark.parametrize("hd", ac.FP32_HD)
def test_emulation_passes_every_check_fp32(hd):
    for N in (1, 17, 50, 197):
        for c in cases_at(N, hd, F32):
            rep = ac.check_all(c, ac.emu_eval(c))
            rep.assert_ok()
            for n, v in rep.worst.items():
                assert v <= ac.K[n] / 4, (c["tag"], n, v)


def test_k_is_derived_from_k_ref():
    assert set(ac.K) == set(ac.K_REF) == {p + "." + n for p in ("bf16", "fp32") for n in ac.CHECKS}
    for n, k in ac.K.items():
        assert k >= 16 and k >= 4 * ac.K_REF[n] and k & (k - 1) == 0 and (k == 16 or k < 8 * ac.K_REF[n])
        assert ac.K_REF[n] == max(ac.K_REF_CPU[n], ac.K_REF_GPU[n])
    assert all(v <= 1.0 for v in ac.U_REF.values())


def test_normaliser_table_covers_every_family():
    assert set(ac.NORMALISER) == {ac.family_of(dt, N, hd) for dt in (BF, F32) for N in (1, 256, 257) for hd in (32, 64)}
    assert [ac.nkt_of(N) for N in (1, 32, 33, 160, 161, 192, 193, 256)] == [2, 2, 4, 10, 12, 12, 14, 16]
    assert {ac.nkt_of(N) for N in ac.ONE_PER_BUCKET} == set(range(2, 17, 2))
    assert {ac.nkt_of(N) for N in ac.whole_head_edges()} == set(range(2, 17, 2))


# wrong variant -> (the family that must catch it, its arguments, the checks that must ALL fail there)
EXPECT = {
    "drop_last_key": ("uniform", {"s0": 0}, {"lse"}),
    "dup_key": ("uniform", {"s0": 0}, {"lse"}),
    "pad_leak": ("uniform", {"s0": -1}, {"o", "lse"}),
    "swap_v": ("onehot", {}, {"o"}),
    "wrong_scale": ("uniform", {"s0": 1}, {"lse"}),
    "lse_no_max": ("gauss", {"scale": 1.5}, {"lse"}),
    "lse_base2": ("gauss", {"scale": 1.5}, {"lse"}),
    "row_dup": ("gauss", {"scale": 1.5}, {"o", "lse"}),
    "last_strip": ("gauss", {"scale": 1.5}, {"o", "dq", "dk", "dv"}),
    "head_swap": ("gauss", {"scale": 1.5}, {"o"}),
    "no_delta": ("gauss", {"scale": 1.5}, {"dq", "dk"}),
    "dk_no_scale": ("gauss", {"scale": 1.5}, {"dk"}),
    "dq_dk_exchanged": ("gauss", {"scale": 1.5}, {"dq", "dk"}),
    "lse_neighbour": ("gauss", {"scale": 1.5}, {"dq", "dk", "dv"}),
    "dv_wrong_head": ("gauss", {"scale": 1.5}, {"dv"}),
}


def test_every_mutation_and_every_check_is_covered():
    assert set(EXPECT) == set(ac.MUTATIONS) and len(ac.MUTATIONS) >= 15
    assert set().union(*(e[2] for e in EXPECT.values())) == set(ac.CHECKS)


@pytest.mark.parametrize("mut", ac.MUTATIONS)
@pytest.mark.parametrize("N,hd", [(50, 32), (197, 32), (197, 64), (300, 32), (512, 64)])
def test_wrong_variant_is_caught(mut, N, hd):
    family, kw, checks = EXPECT[mut]
    c = ac.make_case(family, 2, N, 2, hd, BF, seed=5, **kw)
    ac.check_all(c, ac.emu_eval(c)).assert_ok()
    rep = ac.check_all(c, ac.emu_eval(c, mut=mut))
    assert checks <= set(rep.names()), (mut, c["tag"], rep.names(), rep.failed[:5])


@pytest.mark.parametrize("mut", ["drop_last_key", "dup_key", "pad_leak", "last_strip", "no_delta", "dk_no_scale",
                                 "lse_base2", "head_swap"])
def test_wrong_variant_is_caught_on_the_fp32_path(mut):
    family, kw, checks = EXPECT[mut]
    c = ac.make_case(family, 2, 50, 2, 48, F32, seed=5, **kw)
    ac.check_all(c, ac.emu_eval(c)).assert_ok()
    rep = ac.check_all(c, ac.emu_eval(c, mut=mut))
    assert checks <= set(rep.names()), (mut, rep.names(), rep.failed[:5])


@pytest.mark.parametrize("hd", [32, 64])
def test_padded_key_leak_is_caught_at_every_n(hd):
    """uniform family, every N in 1 ... 256: with the common score 0 the leaked zero key is one key more (lse off by
    log((N + 1) / N) against a 2^-24 bound); with the common score about -32 it takes over the whole softmax and O
    collapses as well.  (With the common score about +32 the leaked key weighs e^-32: nothing can see it, and nothing
    depends on it.)"""
    missed = []
    for N in range(1, 257):
        for s0, checks in ((0, {"lse"}), (-1, {"o", "lse"})):
            c = ac.make_case("uniform", 1, N, 2, hd, BF, s0=s0)
            ok = ac.check_all(c, ac.emu_eval(c, backward=False))
            bad = ac.check_all(c, ac.emu_eval(c, mut="pad_leak", backward=False))
            if ok.failed or not checks <= set(bad.names()):
                missed.append((N, s0, ok.failed, bad.names()))
    assert not missed, missed[:10]


@pytest.mark.parametrize("scale", [1.5, 3.0])
def test_padded_key_leak_is_invisible_to_gauss_at_hd32(scale):
    """the documented gap: random operands at N = 197 do not see the leak under the sum-of-rounded-probabilities
    convention — not under these per-element bounds, so certainly not under a global max-norm tolerance.  If this
    test ever fails, the gauss family has become sharper than claimed: update the module docstring, nothing else."""
    c = ac.make_case("gauss", 2, 197, 3, 32, BF, seed=3, scale=scale)
    rep = ac.check_all(c, ac.emu_eval(c, mut="pad_leak", backward=False))
    assert not rep.failed, rep.failed[:5]
