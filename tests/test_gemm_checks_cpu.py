"""Proof that the GEMM checks of tests/gemm_checks.py bite (no GPU): the fp32 emulation (chunked MFMA sums, split-K
slabs, fp32 epilogues; the generic kernel as an fmaf chain) passes every check in every input family on a reduced
case list, and each deliberately wrong variant of it (gemm_checks.MUTATIONS) fails the check named for it.

The reduced list keeps what each slip needs in order to show: ragged M and N (130 x 136: a second, 8-column tile),
N % 8 != 0 on the fp32 output, alpha != 1, ldr != ldc > N, a non-zero initial C and colsum_a (accumulate), K = 1000
on the TN route (four slabs, a ragged last K-tile), M = 300 for the column statistics (three 128-row blocks, the
last of 44 rows), ReLU with and without aux, a bf16 output (truncation), the GELU pair in all three forms.

What the global norm of the existing tests (rel_err < 8e-3 over the whole matrix, tests/test_gpu_ops.py) would have
passed — NORM_BLIND below, asserted by test_wrong_variant_is_caught on the case named there: the bias shifted by four
columns on the last tile (8 wrong elements of 258 x 264), one 8-column chunk taken from its neighbour (8 of 10^6), the
duplicated last row (1 of 32513), the tanh form of GELU, the truncated bf16 output and the store past N (which no
comparison of C can see at all) — the first three at the sizes where the norm goes blind, rel = sqrt(2 f) < 8e-3 for
a fraction f of wrong elements.  The column statistics
(three variants) are compared by no norm of C either.  The others (alpha, bias twice, accumulate, dropped K chunk or
slab, ...) move the whole matrix and fail the norm as well."""
import pytest
import torch

import gemm_checks as gc
from gemm_checks import (ADD_AUX, AFFINE, BF, BIAS, BIAS_GELU, BIAS_GELU_GRAD, BIAS_RESIDUAL, DGELU, F32, MUL_AUX, NONE,
                         spec)


def cpu_specs():
    for fam in gc.FAMILIES:
        for epi in range(7):
            yield spec(130, 136, 128, "nt", BF, BF if epi != BIAS_RESIDUAL else F32, epi, 0.5, family=fam, seed=epi)
            yield spec(129, 132, 64, "nt", BF, F32, epi, -2.0, family=fam, seed=epi)
            yield spec(65, 63, 33, "nn", F32, F32, epi, 0.5, family=fam, seed=epi)
            yield spec(5, 65, 17, "tt", BF, BF, epi, 1.0, family=fam, seed=epi)
        yield spec(129, 132, 128, "nt", BF, F32, NONE, 0.5, acc=True, family=fam)
        yield spec(64, 63, 33, "tn", F32, F32, NONE, -2.0, acc=True, colsum=True, batch=(1, 1), family=fam)
        yield spec(5, 65, 17, "nn", BF, F32, NONE, 0.5, acc=True, batch=(2, 3), family=fam)
        yield spec(72, 136, 1000, "tn", BF, F32, NONE, 0.5, acc=True, colsum=True, family=fam)
        yield spec(300, 136, 64, "nt", BF, BF, NONE, 0.5, colstats=True, family=fam)
        yield spec(300, 136, 128, "nt", BF, BF, ADD_AUX, -2.0, family=fam)
        for relu in (False, True):
            for aux in (False, True):
                yield spec(130, 136, 64, "nt", BF, BF, AFFINE, 0.5, relu=relu, aux=aux, family=fam)
    # the table form of the GELU pair (256-wide tile) and the split-K plans of the 256 x 256 TN kernel
    for fam in ("gauss", "onehot"):
        for epi in (BIAS_GELU, BIAS_GELU_GRAD):
            yield spec(300, 264, 64, "nt", BF, BF, epi, 1.0, family=fam)


CASES = [gc.make_case(s) for s in cpu_specs()]
TABLE = {"gelu": "table", "splits": 1, "kind": "nt256"}


def run_one(case, mut=None):
    s = case["spec"]
    if s["M"] == 300 and s["epi"] in (BIAS_GELU, BIAS_GELU_GRAD):       # below 128 tiles the heuristic says nt128:
        outs = gc.emulate(case, 1, False, "table", mut)                  # judge the table form by hand
        return gc.check_case(case, outs, 1, "table"), outs
    return gc.emulate_and_check(case, mut=mut)


def run(mut=None, only=None):
    rep = gc.Report()
    for c in CASES:
        if only is None or only(c["spec"]):
            rep.merge(run_one(c, mut)[0])
    return rep


@pytest.mark.parametrize("family", gc.FAMILIES)
def test_emulation_passes_every_check(family):
    """... with a factor 4 to spare: k = max(16, 4 k_ref)"""
    rep = run(only=lambda s: s["family"] == family)
    print(family, {n: round(v, 3) for n, v in rep.worst.items()})
    rep.assert_ok()
    for n, v in rep.worst.items():
        assert v <= gc.K[n] / 4, (n, v)


def test_k_is_derived_from_k_ref():
    assert set(gc.K) == set(gc.CHECKS) == set(gc.K_REF)
    for n in gc.CHECKS:
        k = gc.K[n]
        assert gc.K_REF[n] == max(gc.K_REF_CPU[n], gc.K_REF_GPU.get(n, 0.0))
        assert k >= 16 and k >= 4 * gc.K_REF[n] and k & (k - 1) == 0 and (k == 16 or k < 8 * gc.K_REF[n])
    assert [gc.acc_class(*a) for a in ((64, 1), (448, 1), (512, 1), (4096, 1), (32768, 1), (32768, 128), (65536, 256), (0, 1))] \
        == ["acc_L16", "acc_L16", "acc_L128", "acc_L1024", "acc_Lbig", "acc_L1024", "acc_L1024", "acc_L16"]


def test_gelu_constants_are_measured():
    """c_g, c_d = 4 x the worst ratio of the fp32 torch restatement, rounded up to a power of two; the table's bound
    is the one of test_gelu_table_accuracy_cpu, and the table's emulation meets the copy of it on that test's grid"""
    for form, (wg, wd) in gc.GELU_WORST.items():
        mg, md = gc.measure_gelu_constants(form)
        print(form, mg, md)
        assert abs(mg - wg) < 0.02 * wg and abs(md - wd) < 0.02 * wd, (form, mg, md)
        cg, cd = gc.GELU_C[form]
        assert 4 * wg <= cg < 8 * wg and 4 * wd <= cd < 8 * wd
    g = torch.Generator().manual_seed(0)
    u = torch.cat([2.0 * torch.randn(400000, generator=g), 1e-4 * torch.randn(1000, generator=g),
                   40.0 * torch.randn(1000, generator=g), torch.tensor(gc.SPECIAL_U + (15.9375,))])
    gg, dd = gc.gelu_table32(u)
    assert bool(((gg.double() - gc.gelu64(u)).abs() <= gc.table_bound_g(u)).all())
    assert float((dd.double() - gc.dgelu64(u)).abs().max()) < gc._table_test().DGELU_ABS


def test_the_listed_mutations_are_all_there():
    assert len(gc.MUTATIONS) >= 24 and set(gc.MUTATIONS.values()) <= {"C", "out2", "colsum", "colstats", "guard"}


# the variants the old global norm would have passed, each with the case that shows it
NORM_BLIND = {
    "bias_shifted_4_columns_last_tile": spec(258, 264, 64, "nt", BF, BF, BIAS, 0.5, family="gauss"),     # 8 elements
    "chunk_from_neighbour": spec(1026, 1032, 64, "nt", BF, BF, BIAS, 0.5, family="gauss"),               # 8 of 1e6
    "last_row_duplicated": spec(32513, 8, 64, "nt", BF, BF, BIAS, 0.5, family="gauss"),                  # 1 row of 32513
    "tanh_gelu": spec(130, 136, 128, "nt", BF, BF, BIAS_GELU, 0.5, family="gauss", seed=BIAS_GELU),
    "bf16_truncated": spec(130, 136, 128, "nt", BF, BF, BIAS, 0.5, family="gauss", seed=BIAS),
    "store_past_n": spec(130, 136, 128, "nt", BF, BF, BIAS, 0.5, family="gauss", seed=BIAS),
}


@pytest.mark.parametrize("mut", sorted(gc.MUTATIONS))
def test_wrong_variant_is_caught(mut):
    expect = gc.MUTATIONS[mut]
    rep = run(mut)
    assert expect in rep.names(), (mut, expect, rep.names(), rep.failed[:3])
    if mut in NORM_BLIND:
        case = gc.make_case(NORM_BLIND[mut])
        r, outs = run_one(case, mut)
        name = "out2" if expect == "out2" else "C"
        old = gc.old_rel_err(case, outs, name)
        print(mut, "old global rel_err %.2e" % old)
        assert expect in r.names() and old < 8e-3, (mut, r.names(), old)


def test_old_norm_sees_the_gross_variants():
    """... and only those: the docstring's other half"""
    case = gc.make_case(spec(130, 136, 128, "nt", BF, BF, BIAS, 0.5, family="gauss", seed=BIAS))
    for mut in ("alpha_dropped", "bias_twice", "bias_before_alpha", "last_k_chunk_dropped"):
        _, outs = run_one(case, mut)
        assert gc.old_rel_err(case, outs) > 8e-3, mut


def test_case_lists_are_reproducible():
    s = spec(130, 136, 128, "nt", BF, BF, AFFINE, 0.5, relu=True, family="massive")
    a, b = gc.make_case(s), gc.make_case(s)
    assert all(torch.equal(a[k], b[k]) for k in ("A", "B", "bias", "aux", "scale"))
    assert float(a["scale"][0]) < 0 and float(a["scale"][1]) == 0
    w = a["win"]
    assert torch.equal(w["A"].view().float(), a["A"]) and bool(w["A"].buf[w["A"].outside()].isnan().all())
    assert a["ldc"] > 136 and a["ldc"] % 8 == 0 and a["ldr"] != a["ldc"] and w["A"].strides[2] > 128
    assert bool((w["C"].buf == gc.SENTINEL).all())
    c = gc.make_case(spec(64, 64, 128, "nt", BF, BF, NONE, 1.0, family="cancel"))
    assert float((c["A"].double() @ c["B"].double()).abs().max()) == 0.0
    o = gc.make_case(spec(130, 136, 128, "nt", BF, BF, BIAS_GELU, 1.0, family="onehot"))
    u = (o["A"].double() @ o["B"].double() + o["bias"].double()).reshape(-1)
    assert all(bool((u == v).any()) for v in (0.0, 2.0 ** -12, -2.0 ** -12, 16.0, -16.0, 30.0, -30.0, 9984.0, -9984.0))
    assert len(gc.groups(gc.gpu_specs())) > 40


def test_route_labels():
    r = gc.route
    assert r(spec(65, 63, 33, "nn", F32, F32))["kind"] == "generic"
    assert r(spec(250, 264, 448, "nt"))["kind"] == "nt128"
    a = r(spec(300, 264, 320, "nt", colstats=True))
    assert (a["kind"], a["nj"], a["stats"]) == ("nt256", 3, True) and r(spec(300, 128, 64, "nt", epi=ADD_AUX))["nj"] == 2
    assert r(spec(1500, 512, 64, "nt", epi=ADD_AUX, cus=8))["nj"] == 4
    b = r(spec(16383, 768, 64, "nt", epi=BIAS_GELU))
    assert (b["nj"], b["table"], b["streaming"], b["gelu"]) == (4, True, False, "table")
    assert r(spec(16383, 512, 64, "nt", epi=BIAS_GELU))["nj"] == 3 and r(spec(32513, 200, 64, "nt", epi=BIAS_GELU))["streaming"]
    assert [r(spec(64, 64, k, "tn", BF, F32))["reduce"] for k in (8192, 32768, 65536)] == ["wide4", "wide16", "wide16"]
    assert [r(spec(64, 64, k, "tn", BF, F32))["splits"] for k in (8192, 32768, 65536)] == [32, 128, 256]
    t = r(spec(272, 248, 1088, "tn", BF, F32))
    assert (t["kind"], t["partial"], t["splits"]) == ("tn256", True, 2)
    assert r(spec(256, 256, 16384, "tn", BF, F32))["splits"] == 32 and r(spec(256, 256, 1024, "tn", BF, F32))["splits"] == 2
