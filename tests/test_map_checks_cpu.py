"""Proof that the map / layout checks of tests/map_checks.py bite (no GPU): the plain fp32 torch evaluation of each
formula passes every check on a reduced case list with a factor 4 to spare, and each deliberately wrong variant of
it (map_checks.MUTATIONS) fails the check the table names for it on at least one case of that list.

The reduced list keeps what each slip needs in order to show: an odd and an even H and W (the pool's output size,
the stride-2 centre and parity), border windows with all-negative data (the pad), ties (`quarter`: first against
last maximum), exact zeros and -0.0 in x (masks on x > 0, the sign-clearing ReLU), a length that is not a multiple
of 4 (the momentum update's tail), three images (batch stride), k > 1 and C > one chunk (the scatter's index and the
bias), and M > 262144 rows for the depth head (the second sweep of its grid)."""
import pytest
import torch

import map_checks as mc

F32, BF = torch.float32, torch.bfloat16


def specs(kind):
    for dt in (F32, BF):
        v = mc.V(dt)
        if kind == "bilinear":
            for s in ((1, 1, 1, v), (2, 1, 5, v), (2, 5, 1, v), (2, 3, 5, 2 * v), (1, 4, 6, v)):
                for f in ("gauss", "integers"):
                    yield (f,) + s + (dt,)
        elif kind == "pool3":
            for m in ((1, 1, 5), (2, 5, 1), (2, 7, 9), (2, 12, 10)):
                for C in (v, 3):
                    for f in ("gauss", "quarter", "negative", "integers"):
                        yield (f,) + m + (C, dt)
        elif kind == "pool2":
            for f in ("gauss", "quarter", "negative"):
                yield (f, 2, 4, 6, v, dt)
        elif kind == "avg":
            for HW in (1, 4, 49):
                for C in (3, 8):
                    for f in ("gauss", "negative", "integers"):
                        yield (f, 3, HW, C, dt)
        elif kind == "im2col":
            for stride in (1, 2):
                for H, W in ((1, 6), (7, 9), (8, 8), (8, 9)):
                    for ld in (9 * v, 9 * v + 24):
                        for f in ("signed_zero", "gauss", "integers"):
                            yield (f, 2, H, W, v, stride, ld, int(f != "gauss"), dt)
        elif kind == "stem":
            for s in ((2, 7, 9), (1, 8, 6)):
                yield s + (dt,)
        elif kind == "sub":
            for s in ((2, 7, 9, 2 * v), (2, 8, 6, v)):
                yield ("signed_zero",) + s + (dt,)
        elif kind == "shuffle":
            for s in ((1, 1, 1, 2, v), (2, 5, 6, 2, 24), (1, 2, 3, 4, 2 * v)):
                for f in ("gauss", "integers"):
                    yield (f,) + s + (dt,)
        elif kind == "tokens":
            yield ("signed_zero", 2, 5, 12, dt)
            yield ("gauss", 1, 1, 4, dt)
        elif kind == "eltwise":
            for f in ("gauss", "signed_zero", "grid"):
                yield (f, 257 * v, dt)
        elif kind == "head":
            for f, acc in (("gauss", True), ("signed_zero", False), ("quarter", False)):
                yield (f, 240, 32, dt, acc)
            if dt == F32:
                yield ("gauss",) + mc.HEAD_LONG + (dt, False)
        elif kind == "ema" and dt == F32:
            for n in (3, 4, 1025):
                for m in mc.EMA_M:
                    for f in ("gauss", "integers"):
                        yield (f, n, m)


CASES = {kind: [mc.make(kind, a) for a in specs(kind)] for kind in mc.KINDS}


def run(kind, mut=None):
    rep = mc.Report()
    for c in CASES[kind]:
        rep.merge(mc.run_check(c, mc.evaluate(c, mut)))
    return rep


@pytest.mark.parametrize("kind", sorted(mc.KINDS))
def test_fp32_evaluation_passes_every_check(kind):
    """... the bounded ones with a factor 4 to spare: k = max(16, 4 k_ref)"""
    rep = run(kind)
    print(kind, {n: round(v, 3) for n, v in rep.worst.items()})
    rep.assert_ok()
    for n, v in rep.worst.items():
        assert v <= (mc.K[n] / 4 if n in mc.K else 0.0), (n, v)


def test_every_check_is_exercised():
    seen = set()
    for kind in mc.KINDS:
        seen |= set(run(kind).worst)
    assert seen == set(mc.BOUNDED) | set(mc.EXACT), seen ^ (set(mc.BOUNDED) | set(mc.EXACT))


def test_k_is_derived_from_k_ref():
    assert set(mc.K) == set(mc.CHECKS) == set(mc.K_REF) == set(mc.K_REF_CPU)
    for n in mc.CHECKS:
        k = mc.K[n]
        assert mc.K_REF[n] == max(mc.K_REF_CPU[n], mc.K_REF_GPU.get(n, 0.0))
        assert k >= 16 and k >= 4 * mc.K_REF[n] and k & (k - 1) == 0 and (k == 16 or k < 8 * mc.K_REF[n])


def test_the_listed_mutations_are_all_there():
    assert len(mc.MUTATIONS) >= 30
    assert all(kind in mc.KINDS and chk in mc.BOUNDED + mc.EXACT for kind, chk in mc.MUTATIONS.values())


@pytest.mark.parametrize("mut", sorted(mc.MUTATIONS))
def test_wrong_variant_is_caught(mut):
    kind, expect = mc.MUTATIONS[mut]
    rep = run(kind, mut)
    assert expect in rep.names(), (mut, expect, rep.names(), rep.failed[:3])


def test_bilinear_matrices_are_the_interpolation():
    """the tap matrices behind the bilinear mags reproduce F.interpolate and its gradient"""
    for c in CASES["bilinear"]:
        B, H, W, C = c["shape"]
        r = mc.bilinear_ref(c)
        Ay, Ax = mc.bl_matrix(H)[0], mc.bl_matrix(W)[0]
        y = torch.einsum("oh,bhwc,pw->bopc", Ay, c["x"].double(), Ax)
        dx = torch.einsum("oh,bopc,pw->bhwc", Ay, c["dy"].double(), Ax)
        assert float((y - r["y"]).abs().max()) <= 1e-13 * (1 + float(r["t_y"].max()))
        assert float((dx - r["dx"]).abs().max()) <= 1e-13 * (1 + float(r["t_dx"].max()))
        assert bool((r["t_y"] >= r["y"].abs() - 1e-12).all()) and bool((r["s_y"] >= 0).all())


def test_signed_zero_and_nan_are_seen():
    """`same` compares bits: -0.0 where +0.0 is wanted fails; a NaN fails a bounded check"""
    rep = mc.Report()
    rep.same("add", torch.tensor([-0.0]), torch.tensor([0.0]))
    rep.same("add", torch.zeros(2), torch.zeros(3))
    rep.bounded("ema", torch.tensor([float("nan")]), torch.ones(1, dtype=torch.float64), torch.ones(1, dtype=torch.float64))
    assert len(rep.failed) == 3 and rep.names() == ["add", "ema"]


def test_pool_reference_follows_aten_on_nan():
    """F.max_pool2d: a NaN anywhere in a window is the output and the arg points at it"""
    for pos in (0, 4, 8):
        x = torch.arange(9.0).view(1, 3, 3, 1).repeat(1, 1, 1, 2)
        x[0, pos // 3, pos % 3, 0] = float("nan")
        y, arg = mc.pool3_ref(x[:, :, :, :])
        # window (1, 1) of a 3 x 3 map covers rows / columns 1 .. 2 only; window (0, 0) rows / columns 0 .. 1
        assert y.shape == (1, 2, 2, 2)
        inside = {0: [(0, 0)], 4: [(0, 0), (0, 1), (1, 0), (1, 1)], 8: [(1, 1)]}[pos]
        for oy in range(2):
            for ox in range(2):
                assert bool(torch.isnan(y[0, oy, ox, 0])) == ((oy, ox) in inside)
                if (oy, ox) in inside:
                    assert int(arg[0, oy, ox, 0]) == (pos // 3 - (2 * oy - 1)) * 3 + (pos % 3 - (2 * ox - 1))
        assert not bool(torch.isnan(y[..., 1]).any())


def test_case_lists_are_reproducible():
    a, b = mc.pool3_case("quarter", 2, 7, 9, 8, BF), mc.pool3_case("quarter", 2, 7, 9, 8, BF)
    assert all(torch.equal(a[k], b[k]) for k in a if torch.is_tensor(a[k]))
    assert bool((mc.fam("negative", (64,), mc._gen(1)) < 0).all())
    z = mc.fam("signed_zero", (4096,), mc._gen(2))
    assert bool(((z == 0) & torch.signbit(z)).any()) and bool(((z == 0) & ~torch.signbit(z)).any())
    for kind in mc.KINDS:
        assert len(mc.gpu_specs(kind)) > 0
    assert mc.HEAD_LONG[0] > mc.HEAD_GRID_ROWS
