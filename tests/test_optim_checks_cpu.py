"""Proof that the optimizer checks of tests/optim_checks.py bite (no GPU): the plain fp32 torch evaluation of the
AdamW and LARS steps passes every check over the WHOLE case list of the GPU module at the committed k, with a factor 4
to spare, and each deliberately wrong variant of it (optim_checks.MUTATIONS) fails the check the table names for it
on at least one case of that list.

What each slip needs in order to show is in the list: lr wd about 1e-3 (decay after the update: small's segment 1),
gradients of 1e-9 (where eps sits), t = 1, 2 and 7 (the bias corrections, a step that is off by one), ctl[1] = 0.37
(the clip coefficient in v'), neighbours with different lr, vectors with a weight-decay entry, a segment of more than
32768 elements (the second trip of the LARS norm loop), matrix segments with a zero norm, momentum with a non-zero
buffer, skipped segments inside the range."""
import pytest
import torch

import optim_checks as oc

CASES = {kind: [(grp, a) for grp, a in oc.gpu_specs(kind)] for kind in oc.KINDS}


def run(kind, mut=None, stop_at=None):
    """the evaluation (or its wrong variant) through the checks; stop_at: return at the first case that fails that check"""
    rep = oc.Report()
    for _, a in CASES[kind]:
        c = oc.make(kind, a)
        rep.merge(oc.run_check(c, oc.evaluate(c, mut)))
        if stop_at is not None and stop_at in rep.names():
            break
    return rep


@pytest.fixture(scope="module")
def clean():
    return {kind: run(kind) for kind in oc.KINDS}


@pytest.mark.parametrize("kind", sorted(oc.KINDS))
def test_fp32_evaluation_passes_every_check(kind, clean):
    """... the bounded ones with a factor 4 to spare: k = max(16, 4 k_ref)"""
    rep = clean[kind]
    print(kind, {n: round(v, 3) for n, v in rep.worst.items()})
    rep.assert_ok()
    for n, v in rep.worst.items():
        assert v <= (oc.K[n] / 4 if n in oc.K else 0.0), (n, v)


def test_every_check_is_exercised(clean):
    """the library's runner adds `applied` (the device counter), which no evaluation has"""
    seen = set(clean["adamw"].worst) | set(clean["lars"].worst)
    assert seen == set(oc.CHECKS) | (set(oc.BIT_CHECKS) - {"applied"}), seen
    assert set(clean["lars"].worst) == set(oc.LARS_CHECKS) | {"untouched", "g", "pad_zero"}


def test_k_is_derived_from_k_ref(clean):
    assert set(oc.K) == set(oc.CHECKS) == set(oc.K_REF) == set(oc.K_REF_CPU)
    worst = dict(clean["adamw"].worst, **clean["lars"].worst)
    for n in oc.CHECKS:
        k = oc.K[n]
        assert oc.K_REF[n] == max(oc.K_REF_CPU[n], oc.K_REF_GPU.get(n, 0.0))
        assert k == oc.k_from(oc.K_REF[n])
        assert k >= 16 and k >= 4 * oc.K_REF[n] and k & (k - 1) == 0 and (k == 16 or k < 8 * oc.K_REF[n])
        # the committed CPU figure is what this list gives (another libm may move the last digits)
        assert abs(worst[n] - oc.K_REF_CPU[n]) <= 0.15 * oc.K_REF_CPU[n], (n, worst[n], oc.K_REF_CPU[n])


def test_the_listed_mutations_are_all_there():
    want = {"coupled_decay", "decay_after_update", "eps_inside_sqrt", "eps_before_bias_correction", "bc2_outside_sqrt",
            "t_off_by_one", "b2_for_m", "coef_missing_in_v", "neighbour_lr", "lp_truncated", "lp_from_old_p",
            "write_into_skipped", "wd_on_vector", "q_on_vector", "q_from_g_norm", "norm_first_32768_only",
            "zero_norm_gives_0", "momentum_on_dp", "p_minus_lr_dp"}
    assert want <= set(oc.MUTATIONS)
    assert all(kind in oc.KINDS and chk in oc.CHECKS + oc.BIT_CHECKS for kind, chk in oc.MUTATIONS.values())


@pytest.mark.parametrize("mut", sorted(oc.MUTATIONS))
def test_wrong_variant_is_caught(mut):
    kind, expect = oc.MUTATIONS[mut]
    rep = run(kind, mut, stop_at=expect)
    assert expect in rep.names(), (mut, expect, rep.names(), rep.failed[:3])
    print(mut, "caught by", expect, "first at:", [f for f in rep.failed if (" %s:" % expect) in f][0][:160])


def test_the_slack_is_needed_and_is_the_derived_one():
    """Trap 1: without the bias-correction slack the CORRECT fp32 evaluation exceeds 16 x 2^-24 mag on adamw_p at
    b2 = 0.999, t = 2 — and passes with it: the term is there for a reason and is not folded into k"""
    h = (0.9, 0.999, 2, 1e-8, "host", 1.0)
    c = oc.adamw_case("long", "gauss", h)
    o = oc.adamw_eval(c)
    r = oc.adamw_ref(c)
    act = r["act"]
    with_slack, without = oc.Report(measure=True), oc.Report(measure=True)
    with_slack.ratio("adamw_p", o["p"][act], r["p"][act], r["mag_p"][act], slack=r["slack_p"][act])
    without.ratio("adamw_p", o["p"][act], r["p"][act], r["mag_p"][act])
    print("adamw_p at b2 = 0.999, t = 2: %.2f with the slack, %.2f without" % (with_slack.worst["adamw_p"], without.worst["adamw_p"]))
    assert with_slack.worst["adamw_p"] <= oc.K["adamw_p"] / 4 < oc.K["adamw_p"] < without.worst["adamw_p"]
    b1, b2 = oc.f32r(0.9), oc.f32r(0.999)
    want = r["upd"].abs() * 2.0 ** -23 * (b1 ** 2 / (1 - b1 ** 2) + 0.5 * b2 ** 2 / (1 - b2 ** 2))
    assert torch.equal(r["slack_p"], want)


def test_reference_is_torch_adamw_and_the_reference_lars():
    """the fp64 formulae are torch.optim.AdamW's and moco-v3's LARS: one step of each in float64 on the small layout
    (double betas: torch's own), to 1e-12"""
    c = oc.adamw_case("small", "gauss", (0.9, 0.999, 7, 1e-8, "host", 1.0))
    r = oc.adamw_ref(c, double_betas=True)
    ps = []
    for s, (a, b) in enumerate(zip(c["start"][:-1], c["start"][1:])):
        p = torch.nn.Parameter(c["p"][a:b].double())
        p.grad = c["g"][a:b].double()
        opt = torch.optim.AdamW([p], lr=oc.f32r(c["lr"][s]), betas=(0.9, 0.999), eps=oc.f32r(1e-8),
                                weight_decay=oc.f32r(c["wd"][s]))
        opt.state[p] = {"step": torch.tensor(6.0), "exp_avg": c["m"][a:b].double().clone(),
                        "exp_avg_sq": c["v"][a:b].double().clone()}
        opt.step()
        ps.append(p.detach())
    assert float((torch.cat(ps) - r["p"]).abs().max()) <= 1e-12
    c = oc.lars_case("small", "gauss", (1e-2, 0.9), False)
    r = oc.lars_ref(c)
    for s, (a, b) in enumerate(zip(c["start"][:-1], c["start"][1:])):
        p, g, mu = c["p"][a:b].double(), c["g"][a:b].double(), c["mu"][a:b].double()
        if bool(c["mat"][s]):       # Models/moco_v3/moco/optimizer.py:18-43
            g = g + oc.f32r(c["wd"][s]) * p
            pn, un = p.norm(), g.norm()
            g = g * torch.where(pn > 0, torch.where(un > 0, oc.f32r(oc.TRUST) * pn / un, 1.0), 1.0)
        mu = mu * oc.f32r(0.9) + g
        assert float((p - oc.f32r(c["lr"][s]) * mu - r["p"][a:b]).abs().max()) <= 1e-12
        assert float((mu - r["mu"][a:b]).abs().max()) <= 1e-12


def test_kernel_order_sum_is_a_sum():
    """the fp32 sum in the kernels' order against fp64, below, at and above one trip of 32 x 1024 elements"""
    for n in (64, 1088, 32768, 33344, 70000):
        x = torch.randn(n, generator=oc._gen(9, n))
        s, want = float(oc.kernel_order_sumsq(x)), float((x.double() ** 2).sum())
        assert abs(s - want) <= 8 * oc.EPS32 * want, (n, s, want)
    x = torch.zeros(33344)
    x[32768:] = 1.0
    assert float(oc.kernel_order_sumsq(x)) == 576.0


def test_case_lists_hold_what_the_issue_asks_for():
    hy = oc.adamw_hypers()
    for b in oc.BETAS:
        for mode in ("host", "dev"):
            mine = [h for h in hy if h[:2] == b and h[4] == mode]
            assert {h[2] for h in mine} == set(oc.STEPS) and {h[3] for h in mine} == set(oc.EPSES)
        assert {h[5] for h in hy if h[:2] == b and h[4] == "dev"} == set(oc.COEFS)
    ad = [a for _, a in CASES["adamw"]]
    assert {a[1] for a in ad} == set(oc.ADAMW_FAMILIES) and {a[0] for a in ad} == set(oc.ADAMW_LAYOUTS)
    ranges = {(a[0],) + tuple(a[3:]) for a in ad if len(a) > 3}
    assert ("small", 1152, 1280) in ranges and ("long", 64, 37632) in ranges and ("crowded", 64, 128) in ranges
    la = [a for _, a in CASES["lars"]]
    assert {a[0] for a in la} == set(oc.LARS_LAYOUTS) and {a[2] for a in la} == set(oc.LARS_HYPERS)
    assert {a[3] for a in la} == {True, False} and any(len(a) > 4 for a in la)
    many = oc.LAYOUTS["many"]
    assert len(many["start"]) == 301 and {b - a for a, b in zip(many["start"][:-1], many["start"][1:])} == {64, 128}
    for lay in oc.LAYOUTS.values():
        assert lay["start"][-1] <= 200 * 1024 and lay["tail"]
    assert all(any(w == 0 for w in oc.LAYOUTS[n]["wd"]) for n in ("small", "crowded", "long"))
    assert any(a * b > 5e-4 for lay in oc.LAYOUTS.values() for a, b in zip(lay["lr"], lay["wd"]))
    c = oc.adamw_case("crowded", "gauss", hy[0])
    d = oc.adamw_case("crowded", "gauss", hy[0])
    assert all(torch.equal(c[k].view(torch.int32), d[k].view(torch.int32)) for k in ("p", "g", "m", "v"))
    skipped = (c["lr"] < 0)[oc.seg_index(c["start"])]
    assert bool(torch.isnan(c["g"][skipped]).all()) and not bool(torch.isnan(c["g"][~skipped]).any())
    assert bool((c["v"] >= 0).all())
    for fam in oc.ADAMW_FAMILIES:       # well inside the normal fp32 range, squares included
        c = oc.adamw_case("long", fam, hy[0] if fam == "fresh" else hy[5])
        for k in ("g", "m", "v"):
            x = c[k][~torch.isnan(c[k])].double().abs()
            x = x[x > 0]
            e = 1 if k == "v" else 2        # g is squared; m is held to the same, v to its own value
            assert x.numel() == 0 or (float(x.max()) ** e < 1e30 and float(x.min()) ** e * 1e-3 > 1e-36), (fam, k)


def test_beta_rounding_deviation_is_what_the_docstring_says():
    """Trap 2, recorded and not gated on the kernels: what the ABI's float betas cost against double betas"""
    dev = oc.beta_rounding_deviation()
    print({b: {t: float("%.2g" % v) for t, v in d.items()} for b, d in dev.items()})
    for b, d in dev.items():
        assert d[1] < 1e-12             # m = v = 0 before step 1: the betas cancel
        assert d[10] < d[1000] < 5e-5
