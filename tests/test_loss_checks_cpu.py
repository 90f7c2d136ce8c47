"""Proof that the loss checks of tests/loss_checks.py bite (no GPU): the plain fp32 torch evaluation of each formula
passes every check at every case of the GPU module's list with a factor 4 to spare, and each deliberately wrong
variant of it (loss_checks.MUTATIONS) fails the check the table names for it on at least one case of that list.
Also: the restated references equal the package's torch formulations and the closed forms behind the mags equal
autograd; the sign disagreements between the fp32 and fp64 SSI evaluations lie inside the exempt set and the exempt
share stays under its cap; `dyadic` is bit-equal between fp32 and fp64 torch; the `degenerate` images have a
determinant of exactly 0 in fp64."""
import pytest
import torch

import loss_checks as lk

F32, F64 = torch.float32, torch.float64
CASES = {kind: [lk.make(kind, a) for _, a in lk.gpu_specs(kind)] for kind in lk.KINDS}


def run(kind, mut=None):
    rep = lk.Report()
    for c in CASES[kind]:
        rep.merge(lk.run_check(c, lk.evaluate(c, mut)))
    return rep


@pytest.mark.parametrize("kind", sorted(lk.KINDS))
def test_fp32_evaluation_passes_every_check(kind):
    """... the bounded ones with a factor 4 to spare: k = max(16, 4 k_ref)"""
    rep = run(kind)
    print(kind, {n: round(v, 3) for n, v in rep.worst.items()})
    rep.assert_ok()
    for n, v in rep.worst.items():
        assert v <= (lk.K[n] / 4 if n in lk.K else 0.0), (n, v)


def test_every_check_is_exercised():
    seen = set()
    for kind in lk.KINDS:
        seen |= set(run(kind).worst)
    assert seen == set(lk.BOUNDED) | set(lk.EXACT), seen ^ (set(lk.BOUNDED) | set(lk.EXACT))


def test_k_is_derived_from_k_ref():
    assert set(lk.K) == set(lk.CHECKS) == set(lk.K_REF) == set(lk.K_REF_CPU) == set(lk.K_REF_GPU)
    for n in lk.CHECKS:
        k = lk.K[n]
        assert lk.K_REF[n] == max(lk.K_REF_CPU[n], lk.K_REF_GPU[n])
        assert k == lk.k_from(lk.K_REF[n])
        assert k >= 16 and k >= 4 * lk.K_REF[n] and k & (k - 1) == 0 and (k == 16 or k < 8 * lk.K_REF[n])
        assert lk.K_REF[n] <= 16, "a k_ref above 16 means a term is missing from mag"
    assert "%.2f" % lk.K_REF_CPU["ssi_dpred"] in lk.table() and lk.table() in lk.__doc__


def test_recorded_k_ref_is_what_the_cpu_measures():
    worst = lk.measure_k_ref("cpu", log=lambda s: None)
    for n in lk.CHECKS:
        assert worst[n] <= lk.K[n] / 4, (n, worst[n])


def test_the_listed_mutations_are_all_there():
    assert len(lk.MUTATIONS) >= 23
    assert all(kind in lk.KINDS and chk in lk.BOUNDED + lk.EXACT for kind, chk in lk.MUTATIONS.values())
    assert set(lk.EVAL) == set(lk.KINDS)


@pytest.mark.parametrize("mut", sorted(lk.MUTATIONS))
def test_wrong_variant_is_caught(mut):
    kind, expect = lk.MUTATIONS[mut]
    rep = run(kind, mut)
    assert expect in rep.names(), (mut, expect, rep.names(), rep.failed[:3])


# ------------------------------------------------------------------ the references themselves
def test_ssi_restatement_equals_the_package_formulation():
    from ssl4gie_amd import losses as Lm
    for c in CASES["ssi"]:
        p, t = c["pred"].to(F64), c["target"].to(F64)
        mask = t > 0
        s, h = Lm.compute_scale_and_shift(p, t, mask)
        ssi = s.view(-1, 1, 1) * p + h.view(-1, 1, 1)
        want = Lm.mse_loss(ssi, t, mask)
        for k in range(c["scales"] if c["alpha"] > 0 else 0):
            st = 2 ** k
            want = want + c["alpha"] * Lm.gradient_loss(ssi[:, ::st, ::st], t[:, ::st, ::st], mask[:, ::st, ::st])
        r = lk.ssi_ref(c)
        assert abs(float(want) - float(r["loss"])) <= 1e-14 * max(1.0, abs(float(want))), lk.tag_of(c)   # per-image sums first
        assert abs(r["closed_loss"] - float(want)) <= 1e-12 * max(1.0, abs(float(want)))


def test_other_references_equal_the_package_formulations():
    from ssl4gie_amd import losses as Lm
    for c in CASES["dice"]:
        want = Lm.SoftDiceLoss(smooth=lk.f32(lk.DICE_SMOOTH))(c["logits"].to(F64), c["target"].to(F64))
        assert float(want) == float(lk.dice_ref(c)["loss"])
    for c in CASES["nce"]:
        want = Lm.info_nce(c["q"].to(F64), c["k"].to(F64), lk.f32(c["T"]), c["off"])
        got = float(lk.nce_ref(c)["loss"])
        assert abs(float(want) - got) <= 1e-12 * max(1.0, abs(got))      # F.normalize's eps: 1e-12 against its fp32 value
    for c in CASES["softce"]:
        x = c["x"].to(F64)
        fn = Lm.SoftTargetCrossEntropy() if c["form"] == "soft" else Lm.LabelSmoothingCrossEntropy(lk.SMOOTHING)
        want = fn(x, c["t"].to(F64) if c["form"] == "soft" else c["y"])
        assert abs(float(want) - float(lk.softce_ref(c)["loss"])) <= 1e-14 * max(1.0, abs(float(want)))
    for c in CASES["ce"]:
        w = None if c["w"] is None else c["w"].to(F64)
        got = float(lk.ce_formula(c["x"].to(F64), c["t"], w))
        assert abs(got - float(lk.ce_ref(c)["loss"])) <= 1e-13 * max(1.0, abs(got))


def test_closed_forms_behind_the_mags_equal_autograd():
    """pass C of the SSI kernel, the Dice gradient and the InfoNCE projection, each against autograd in fp64; every
    mag is at least the size of what it bounds"""
    for c in CASES["ssi"]:
        r = lk.ssi_ref(c)
        if c["family"] == "perfect_fit" or bool(r["exempt"].any()) and c["family"] != "dyadic":
            continue            # at a near-tie the two differ by the sign term
        top = float(r["dpred"].abs().max())
        assert float((r["closed"] - r["dpred"]).abs().max()) <= 1e-12 * top, lk.tag_of(c)
        assert bool((r["mag"] >= r["dpred"].abs() * (1 - 1e-9)).all())
        assert bool((r["mag"] >= r["mag_dyadic"] * (1 - 1e-9)).all())
    for kind, ref, key in (("dice", lk.dice_ref, "dlogits"), ("nce", lk.nce_ref, "dq")):
        for c in CASES[kind]:
            r = ref(c)
            top = float(r[key].abs().max())
            assert float((r["closed"] - r[key]).abs().max()) <= 1e-10 * top, lk.tag_of(c)
            assert bool((r["mag"] >= r[key].abs() * (1 - 1e-9)).all())


def _pair_signs(p, t, scales):
    """per scale and direction: (sign of the pair difference, both pixels valid) in the dtype of p"""
    m = (t > 0).to(p.dtype)
    s, h, _ = lk.ssi_scale_shift(p, t, m)
    d = m * (s.view(-1, 1, 1) * p + h.view(-1, 1, 1) - t)
    out = []
    for k in range(scales):
        st = 2 ** k
        dk, mk = d[:, ::st, ::st], m[:, ::st, ::st]
        out.append((torch.sign(dk[:, :, 1:] - dk[:, :, :-1]), mk[:, :, 1:] * mk[:, :, :-1] > 0,
                    torch.sign(dk[:, 1:] - dk[:, :-1]), mk[:, 1:] * mk[:, :-1] > 0))
    return out


def test_sign_disagreements_lie_inside_the_exempt_set():
    pairs = flips = 0
    for c in CASES["ssi"]:
        if c["alpha"] == 0 or c["family"] == "perfect_fit":
            continue
        ex = lk.ssi_ref(c)["exempt"]
        a, b = _pair_signs(c["pred"], c["target"], c["scales"]), _pair_signs(c["pred"].to(F64), c["target"].to(F64), c["scales"])
        for k, ((sx, wx, sy, wy), (tx, _, ty, _)) in enumerate(zip(a, b)):
            ek = ex[:, ::2 ** k, ::2 ** k]
            bad_x, bad_y = wx & (sx.to(F64) != tx), wy & (sy.to(F64) != ty)
            pairs += int(wx.sum()) + int(wy.sum())
            flips += int(bad_x.sum()) + int(bad_y.sum())
            if c["family"] == "dyadic":
                assert not bool(bad_x.any()) and not bool(bad_y.any())
                continue
            assert bool((ek[:, :, 1:] & ek[:, :, :-1])[bad_x].all()) and bool((ek[:, 1:] & ek[:, :-1])[bad_y].all()), lk.tag_of(c)
    print("pairs", pairs, "sign disagreements", flips)
    assert pairs > 10000


def test_exempt_share_is_within_the_cap():
    share = {}
    for c in CASES["ssi"]:
        if c["family"] in ("perfect_fit", "dyadic"):
            continue
        v = float(lk.ssi_ref(c)["exempt"].float().mean())
        assert v <= lk.EXEMPT_CAP, lk.tag_of(c)
        assert c["family"] != "narrow" or c["alpha"] == 0
        share[c["family"]] = max(share.get(c["family"], 0.0), v)
    print({f: "%.3f %%" % (100 * v) for f, v in share.items()})
    narrow = lk.ssi_case("narrow", 2, 33, 40, 0.5, 4)
    assert float(lk.ssi_ref(narrow)["exempt"].float().mean()) > lk.EXEMPT_CAP      # why `narrow` runs at alpha = 0


def test_dyadic_family_is_exact():
    for c in CASES["ssi"]:
        if c["family"] != "dyadic":
            continue
        t, p = c["target"], c["pred"]
        m = t > 0
        assert [int(m[:, ::s, ::s].sum()) for s in (1, 2, 4, 8)] == [512, 128, 32, 8]
        assert all(float((p[b] * m[b]).sum()) == 0 and bool((p[b][m[b]].abs() == 1).all()) for b in range(3))
        r, o = lk.ssi_ref(c), lk.ssi_eval(c)
        assert r["zero_pairs"] > 0                  # sign(0) is reached
        assert float(r["det"][0]) == 256.0 ** 2 and float(r["det"][1]) == 128.0 ** 2
        assert torch.equal(o["loss"].to(F64), r["loss"]) and torch.equal(o["dpred"].to(F64), r["dpred"])
        rep = lk.run_check(c, o)
        assert rep.bit_equal["ssi_dyadic"] == (768, 768) and rep.bit_equal["ssi_dyadic_loss"] == (1, 1)


def test_degenerate_images_are_singular_in_fp64():
    seen = 0
    for c in CASES["ssi"]:
        r = lk.ssi_ref(c)
        if c["family"] == "degenerate":
            seen += 1
            m = c["target"] > 0
            assert [int(m[b].sum()) for b in (1, 2, 3)] == [0, 1, 2]
            assert r["det"].tolist()[1:] == [0.0, 0.0, 0.0] and float(r["det"][0]) != 0
            assert float(r["scale"][1:].abs().max()) == 0 and float(r["shift"][1:].abs().max()) == 0
            assert float(r["dpred"][1:].abs().max()) == 0 and float(r["dpred"][0].abs().max()) > 0
            o = lk.ssi_eval(c)
            assert float(o["dpred"][1:].abs().max()) == 0
        if c["shape"][1:] == (1, 1):
            assert bool(r["singular"].all())        # one pixel: a00 a11 == a01^2
    assert seen == 2


def test_case_list_reaches_the_branches_it_is_there_for():
    shapes = {c["shape"] for c in CASES["ssi"]}
    assert any(B > 256 for B, H, W in shapes) and any(H * W > lk.NB * 256 for B, H, W in shapes)
    assert any(H < 8 and H % 2 for B, H, W in shapes) and (2, 1, 1) in shapes
    assert {c["scales"] for c in CASES["ssi"]} == {1, 2, 3, 4} and {c["alpha"] for c in CASES["ssi"]} == {0.0, 0.5, 1.0}
    assert any(B > 256 for B, n in lk.DICE_SHAPES) and any(n > lk.NB * 256 for B, n in lk.DICE_SHAPES)
    assert any(B > lk.CE_TRIP for B, C in lk.CE_SHAPES) and {63, 64, 65} <= {C for B, C in lk.CE_SHAPES}
    assert [lk.nce_plan(N, M)[2] for N, M in lk.NCE_SPC2] == [2, 2]
    assert any(D > lk.BT_MAXBLK and D % 4 for D in lk.BT_DIMS) and any(D > lk.BT_MAXBLK and D % 4 == 0 for D in lk.BT_DIMS)
    zq = [c for c in CASES["nce"] if c["family"] == "zero_query"]
    assert zq and all(bool((c["q"].norm(dim=1) == 0).any()) for c in zq)
    assert any(bool((c["w"][c["t"]] == 0).any()) for c in CASES["ce"] if c["weights"] == "weight0")
    assert any(bool(torch.isinf(c["x"]).any()) for c in CASES["ce"] if c["family"] == "neg_inf")
    mix = [c for c in CASES["softce"] if c["family"] == "mixup"]
    assert any(float((c["t"].sum(1) - 1).abs().max()) > 0.1 for c in mix)
    exact = [c for c in CASES["bt"] if lk.bt_ref(c)["exact"]]
    assert {c["shape"][0] for c in exact} == {1, 129, 256}


def test_case_lists_are_reproducible():
    for kind in lk.KINDS:
        _, a = lk.gpu_specs(kind)[-1]
        x, y = lk.make(kind, a), lk.make(kind, a)
        assert all(torch.equal(x[k], y[k]) for k in x if torch.is_tensor(x[k]))
