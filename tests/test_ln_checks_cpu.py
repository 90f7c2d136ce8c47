"""Proof that the LayerNorm / map LayerNorm / column-sum checks of tests/ln_checks.py bite (no GPU): the plain fp32
torch evaluation of the textbook formulae passes every check on a reduced case list, and each deliberately wrong
variant of it (ln_checks.MUTATIONS) fails the check the table names for it on at least one case of that list.

The reduced list keeps what each slip needs in order to show: column counts that are not a multiple of 256 (the
padded mean), rows past 4096 (the grid-stride loop), var <= eps (`tiny`, `const`: eps outside the root), a
non-zero initial dgamma / dbeta (accumulate), a bf16 dx_lp (truncation), three images (dw over the first only)."""
import pytest
import torch

import ln_checks as lc

F32, BF = torch.float32, torch.bfloat16


def row_cases():
    for family in lc.ROW_FAMILIES:
        for rows, cols in ((5, 4), (37, 260), (397, 768), (300, 384)):
            for i, (yt, dyt, dres, acc) in enumerate(((F32, F32, True, False), (BF, BF, False, True))):
                yield lc.row_case(family, rows, cols, yt, dyt, dres, acc)
    yield lc.row_case("gauss", 4097, 64, BF, BF, True, True)
    yield lc.row_case("integers", 4097, 128, F32, F32, False, False)
    yield lc.row_case("gauss", 1000, 1024, F32, BF, True, False)


def map_cases():
    for family in lc.MAP_FAMILIES:
        for B, M, dtype, acc in ((1, 8, F32, False), (3, 2880, F32, True), (3, 2880, BF, False), (1, 1 << 17, BF, True)):
            yield lc.map_case(family, B, M, dtype, 8, acc)


def colsum_cases():
    for rows, cols, ld in ((37, 130, 130), (333, 6, 14), (1577, 384, 408), (2049, 64, 64), (5, 8, 32)):
        for dtype in (F32, BF):
            yield lc.colsum_case("gauss", rows, cols, ld, dtype, accumulate=ld > cols)
            yield lc.colsum_case("integers", rows, cols, ld, dtype)


ROW, MAP, COLSUM = list(row_cases()), list(map_cases()), list(colsum_cases())


def run(kind, mut=None):
    rep = lc.Report()
    if kind == "row":
        for c in ROW:
            rep.merge(lc.check_row_all(c, lc.fp32_eval(c, mut)))
    elif kind == "map":
        for c in MAP:
            rep.merge(lc.check_map_all(c, lc.fp32_eval_map(c, mut)))
    else:
        for c in COLSUM:
            rep.merge(lc.check_colsum_all(c, lc.fp32_colsum(c, mut)))
    return rep


@pytest.mark.parametrize("kind", ["row", "map", "colsum"])
def test_fp32_evaluation_passes_every_check(kind):
    """... with a factor 4 to spare: k = max(16, 4 k_ref)"""
    rep = run(kind)
    print(kind, {n: round(v, 3) for n, v in rep.worst.items()})
    rep.assert_ok()
    for n, v in rep.worst.items():
        assert v <= lc.K[n] / 4, (n, v)


def test_k_is_derived_from_k_ref():
    assert set(lc.K) == set(lc.CHECKS) == set(lc.K_REF)
    for n in lc.CHECKS:
        k = lc.K[n]
        assert lc.K_REF[n] == max(lc.K_REF_CPU[n], lc.K_REF_GPU.get(n, 0.0))
        assert k >= 16 and k >= 4 * lc.K_REF[n] and k & (k - 1) == 0 and (k == 16 or k < 8 * lc.K_REF[n])


def test_the_listed_mutations_are_all_there():
    assert len(lc.MUTATIONS) >= 24 and all(kind in ("row", "map", "colsum") for kind, _ in lc.MUTATIONS.values())


@pytest.mark.parametrize("mut", sorted(lc.MUTATIONS))
def test_wrong_variant_is_caught(mut):
    kind, expect = lc.MUTATIONS[mut]
    rep = run(kind, mut)
    assert expect in rep.names(), (mut, expect, rep.names(), rep.failed[:3])


@pytest.mark.parametrize("sigmas", [50, 500])
@pytest.mark.parametrize("dtype", [F32, BF], ids=["fp32", "bf16"])
def test_outlier_at_the_pivot(sigmas, dtype):
    """the statistics' bounds are about the MEAN: with one element `sigmas` sigma out at element 0, two passes meet
    them, and so do per-part (count, mean, M2) triples (what mapln_stats_kernel computes); sums about element 0
    (var = E[d^2] - E[d]^2, what it once computed) do not; with the same element at index 1 all do"""
    for B, M in ((1, 1 << 17), (3, 1 << 19)):
        c = lc.map_case("outlier_first_%d" % sigmas, B, M, dtype)
        lc.check_map_all(c, lc.fp32_eval_map(c)).assert_ok()
        lc.check_map_all(c, lc.fp32_eval_map(c, parts=True)).assert_ok()
        rep = lc.check_map_all(c, lc.fp32_eval_map(c, pivot=True))
        print(sigmas, dtype, M, {n: round(v, 1) for n, v in rep.worst.items() if "mean" in n or "var" in n or "rstd" in n})
        assert "map_rstd" in rep.names() and "map_var" in rep.names(), rep.worst
        c = lc.map_case("outlier_elsewhere_%d" % sigmas, B, M, dtype)
        lc.check_map_all(c, lc.fp32_eval_map(c)).assert_ok()
        lc.check_map_all(c, lc.fp32_eval_map(c, pivot=True)).assert_ok()


def test_statistics_by_parts_pass_on_every_map_family():
    rep = lc.Report()
    for c in MAP:
        rep.merge(lc.check_map_all(c, lc.fp32_eval_map(c, parts=True)))
    print({n: round(v, 3) for n, v in rep.worst.items()})
    rep.assert_ok()


def test_case_lists_are_reproducible():
    a, b = lc.row_case("massive", 37, 260, BF, BF, True, True), lc.row_case("massive", 37, 260, BF, BF, True, True)
    assert all(torch.equal(a[k], b[k]) for k in a if torch.is_tensor(a[k]))
    assert float(a["gamma"][0]) == 0.0 and float(a["gamma"][1]) < 0.0
    c = lc.row_case("const", 5, 64)
    assert bool((c["x"] == c["x"][:, :1]).all())
    assert lc.ln_bwd_blocks(4096) == 1024 and lc.ln_bwd_blocks(4097) == 1024 and lc.ln_bwd_blocks(5) == 2
    assert [lc.ln_bwd_blocks(r) for r in lc.GEOMETRY_ROWS[8:]] == [n for n in lc.REDUCE_NPARTS if n < 1024]
