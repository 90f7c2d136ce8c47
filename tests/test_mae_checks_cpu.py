"""Proof that the MAE glue, cast and loss checks of tests/mae_checks.py bite (no GPU): the plain fp32 torch evaluation
of each formula passes every check on a reduced case list with a factor 4 to spare, and each deliberately wrong
variant of it (mae_checks.MUTATIONS) fails the check the table names for it on at least one case of that list.

What each reduced case is there for:
    cast        n = 5 and 1025 (a tail of n % 4 elements for `cast_tail_dropped`), bf16 gauss (half the values round
                up: truncation), `specials` (NaN positions, ties, denormals through `same_cast`)
    transpose   33 x 65 and 45 x 70 (rows != cols: the exchanged edge guard drops the ragged edge), 1 x 33, 33 x 1
    tbatch      all seven matrices in one arena (the sentinel between them), and 65 x 63 alone
    addcast     b given and None, each output alone and both, both operand types
    argsort     `ties` with an all-equal row (an unstable order shows), len_keep 0, 1, L // 4, L (> against >= moves
                one element unless len_keep = L), L on either side of 64
    gather      32 x 48 with p = 16 (H != W: gw = H / p), B = 2 with ids of which only nsel are read (the row stride),
                C = 3 and 4 (the two column orders differ), both orders
    tokens      B = 2 with ids wider than nsel (the stride), signed zeros (bits), pos rows that differ
    dcls        B = 1, 15, 17, 40 (B rounded down to 16 loses rows), accumulate on and off, integers (exact)
    decoder     nkeep = 0, 0 < nkeep < L with more than 8 removed rows (20 - 1 and 16 - 4), nkeep = L (dmask exactly
                0 or the initial value), accumulate on and off, bf16 y
    loss        P = 48 and 192 (a partly filled and a full slot), H != W, norm_pix on and off, pred with and without
                the cls row, the three masks, gpp given and None, gscale 1 and 0.125; `const` (var = 0, r = 10^3) and
                `offset` (the variance cancels) for the norm_pix mags, `tiny` (var of the size of eps: eps outside the
                root), `integers` for the exact per_patch
    u8          every byte value in 3 x 30 x 28, ImageNet statistics (three different channels) and the identity"""
import os

import numpy as np
import pytest
import torch

import mae_checks as mk

F32, BF, F64 = torch.float32, torch.bfloat16, torch.float64
GOLDEN = os.path.join(os.path.dirname(__file__), "golden")


def specs(kind):
    if kind == "cast":
        for dt in (F32, BF):
            for n in (0, 3, 5, 1025):
                for f in ("gauss", "specials"):
                    yield (f, n, dt)
    elif kind == "transpose":
        for dt in (F32, BF):
            for s in ((1, 33), (33, 1), (33, 65), (45, 70)):
                yield ("gauss",) + s + (dt,)
            yield ("specials", 5, 7, dt)
    elif kind == "tbatch":
        yield (mk.TBATCH_MATS,)
        yield ((mk.TBATCH_MATS[1],),)
    elif kind == "addcast":
        for has_b in (0, 1):
            for want, lp in ((1, None), (0, BF), (1, F32), (1, BF)):
                yield ("signed_zero", 1028, has_b, want, lp)
    elif kind == "argsort":
        for L in (1, 63, 65):
            for keep in mk.len_keeps(L):
                for f in ("uniform", "ties", "signed_zero"):
                    yield (f, 3, L, keep)
    elif kind == "gather":
        for dt in (F32, BF):
            for s in ((2, 3, 32, 48, 16), (1, 3, 8, 8, 4), (2, 4, 16, 16, 8)):
                for order in (0, 1):
                    for with_ids in (0, 1):
                        yield ("signed_zero" if with_ids else "gauss",) + s + (order, with_ids, dt)
    elif kind == "tokens":
        for dt in (F32, BF):
            for s in ((1, 1, 4), (2, 3, 8), (2, 5, 252)):
                for with_ids in (0, 1):
                    yield ("signed_zero",) + s + (dt, with_ids)
    elif kind == "dcls":
        for B in (1, 15, 17, 40):
            for acc in (0, 1):
                for f in ("gauss", "integers"):
                    yield (f, B, 132, acc)
    elif kind == "decoder":
        for dt in (F32, BF):
            for s in ((1, 1, 0, 4), (2, 16, 4, 128), (3, 9, 9, 8), (2, 9, 0, 8), (2, 20, 1, 1028)):
                for acc in (0, 1):
                    for f in ("gauss", "integers"):
                        yield (f,) + s + (dt, acc)
    elif kind == "loss":
        for s in ((2, 3, 8, 8, 4), (2, 3, 16, 24, 8)):
            for norm in (0, 1):
                for hc in (0, 1):
                    for i, f in enumerate(mk.LOSS_FAMILIES):
                        for j in range(3):
                            yield (f,) + s + (norm, hc) + mk.LOSS_COMBOS[(2 * i + j + hc) % len(mk.LOSS_COMBOS)]
    elif kind == "u8":
        for s in ((1, 1, 4), (3, 30, 28)):
            for identity in (0, 1):
                yield s + (identity,)


CASES = {kind: [mk.make(kind, a) for a in specs(kind)] for kind in mk.KINDS}


def run(kind, mut=None):
    rep = mk.Report()
    for c in CASES[kind]:
        rep.merge(mk.run_check(c, mk.evaluate(c, mut)))
    return rep


@pytest.mark.parametrize("kind", sorted(mk.KINDS))
def test_fp32_evaluation_passes_every_check(kind):
    """... the bounded ones with a factor 4 to spare: k = max(16, 4 k_ref)"""
    rep = run(kind)
    print(kind, {n: round(v, 3) for n, v in rep.worst.items()})
    rep.assert_ok()
    for n, v in rep.worst.items():
        assert v <= (mk.K[n] / 4 if n in mk.K else 0.0), (n, v)


def test_every_check_is_exercised():
    seen = set()
    for kind in mk.KINDS:
        seen |= set(run(kind).worst)
    assert seen == set(mk.BOUNDED) | set(mk.EXACT), seen ^ (set(mk.BOUNDED) | set(mk.EXACT))


def test_k_is_derived_from_k_ref():
    assert set(mk.K) == set(mk.CHECKS) == set(mk.K_REF) == set(mk.K_REF_CPU) == set(mk.K_REF_GPU)
    for n in mk.CHECKS:
        k = mk.K[n]
        assert mk.K_REF[n] == max(mk.K_REF_CPU[n], mk.K_REF_GPU[n])
        assert k == mk.k_from(mk.K_REF[n])
        assert k >= 16 and k >= 4 * mk.K_REF[n] and k & (k - 1) == 0 and (k == 16 or k < 8 * mk.K_REF[n])


def test_the_listed_mutations_are_all_there():
    assert len(mk.MUTATIONS) >= 23
    assert all(kind in mk.KINDS and chk in mk.BOUNDED + mk.EXACT for kind, chk in mk.MUTATIONS.values())
    assert set(mk.EVAL) == set(mk.KINDS)


@pytest.mark.parametrize("mut", sorted(mk.MUTATIONS))
def test_wrong_variant_is_caught(mut):
    kind, expect = mk.MUTATIONS[mut]
    rep = run(kind, mut)
    assert expect in rep.names(), (mut, expect, rep.names(), rep.failed[:3])


def _npz(name):
    return {k: torch.from_numpy(np.asarray(v)) for k, v in np.load(os.path.join(GOLDEN, name)).items()}


def test_masking_reference_agrees_with_the_fixture():
    g = _npz("g1_masking.npz")
    for pre in ("", "tie_"):
        s, r, m = mk.masking(g[pre + "noise"], 49)
        assert torch.equal(s, g[pre + "ids_shuffle"]) and torch.equal(r, g[pre + "ids_restore"])
        assert torch.equal(m, g[pre + "mask"])


def test_patch_reference_agrees_with_the_fixture():
    g = _npz("g2_patchify.npz")
    for with_ids in (0, 1):
        c = mk.gather_case("gauss", 2, 3, 64, 64, 16, 1, with_ids, F32)
        c["img"] = g["imgs"]
        want = g["patches"] if not with_ids else torch.stack([g["patches"][b, c["ids"][b, :c["nsel"]]] for b in range(2)])
        assert torch.equal(mk.gather_ref(c), want.reshape(-1, 768))
        assert torch.equal(mk.evaluate(c)["out"], want.reshape(-1, 768))
    assert torch.equal(mk.patches_by_index(g["imgs"], 16, 1), g["patches"])


@pytest.mark.parametrize("norm_pix", [0, 1])
def test_loss_reference_agrees_with_the_oracle(norm_pix):
    """value and autograd gradient of oracle/mae_ref.mae_loss in fp64; loss = sum per_patch / sum mask, so the
    gradient is dpred with gpp = 1 / sum mask"""
    from oracle import mae_ref
    c = mk.loss_case("gauss", 2, 3, 16, 16, 8, norm_pix, 0, "random", 1, 1.0)
    msum = float(c["mask"].sum())
    c["gpp"] = torch.full_like(c["mask"], 1.0 / msum)
    r = mk.loss_ref(c)
    cfg = mae_ref.MAEConfig(img_size=16, patch_size=8, norm_pix_loss=bool(norm_pix))
    pred = c["pred"][:, 1:].to(F64).requires_grad_(True)
    loss = mae_ref.mae_loss(cfg, c["img"].to(F64), pred, c["mask"].to(F64))
    g, = torch.autograd.grad(loss, pred)
    assert abs(float(r["pp"].sum() / msum - loss)) <= 1e-12 * float(loss)
    scale = float(c["gpp"][0, 0].to(F64)) * msum         # gpp as rounded to fp32
    assert float((r["dp"] - g * scale).abs().max()) <= 1e-12 * float(g.abs().max())
    assert bool((r["t_pp"] >= r["pp"]).all()) and bool((r["t_dp"] >= r["dp"].abs() * (1 - 1e-12)).all())


def test_cast_comparison_sees_nan_zero_sign_and_denormals():
    """`same_cast`: a NaN against a number fails, -0 for +0 fails, a flushed denormal passes and is counted, a
    denormal turned into the wrong zero fails"""
    x = mk.specials(34)
    want = x.to(BF)
    rep = mk.Report()
    rep.same_cast("cast", want.clone(), x)
    assert not rep.failed and rep.denormal["rne"] > 0 and rep.denormal["zero"] == 0
    flushed = torch.where(mk.is_denormal(x), torch.where(torch.signbit(x), -torch.zeros_like(want), torch.zeros_like(want)), want)
    rep.same_cast("cast", flushed, x)
    assert not rep.failed and rep.denormal["zero"] > 0
    for bad in (torch.where(torch.isnan(want), torch.ones_like(want), want),
                torch.where(want == 0, torch.zeros_like(want), want),
                torch.where(mk.is_denormal(x), torch.zeros_like(want), want)):
        rep = mk.Report()
        rep.same_cast("cast", bad, x)
        assert rep.names() == ["cast"]
    assert float(torch.tensor(0x7f7fffff, dtype=torch.int32).view(F32).to(BF)) == float("inf")


def test_case_lists_are_reproducible():
    a, b = mk.loss_case("const", 2, 3, 8, 8, 4, 1, 1, "random", 1, 0.125), mk.loss_case("const", 2, 3, 8, 8, 4, 1, 1, "random", 1, 0.125)
    assert all(torch.equal(a[k], b[k]) for k in a if torch.is_tensor(a[k]))
    t = mk.patches_by_index(a["img"], 4, 1)
    assert bool((t == t[:, :, :1]).all()) and bool((a["img"] * 4 == (a["img"] * 4).round()).all())
    z = mk.noise_of("ties", 3, 65, mk._gen(2))
    assert bool(((z == 0) & torch.signbit(z)).any()) and bool(((z == 0) & ~torch.signbit(z)).any())
    assert bool((z[0] == z[0, 0]).all())
    for kind in mk.KINDS:
        assert len(mk.gpu_specs(kind)) > 0
    rows = [s[0] * ((s[2] // s[4]) * (s[3] // s[4]) + hc) for s in mk.LOSS_SHAPES for hc in (0, 1)]
    assert any(r % 4 for r in rows)
    assert sorted(set(torch.cat([mk.u8_case(3, 30, 28, 0)["img"].reshape(-1)]).tolist())) == list(range(256))
