"""The split-K plans of the TN (weight-gradient) GEMMs, pinned through the three workspace queries, which need no GPU:
ssl4gie_gemm_workspace_bytes (lone product), ssl4gie_gemm_tn_pair_workspace_bytes, ssl4gie_gemm_tn_group_workspace_bytes.
The expected byte counts come from the split rules as restated in tests/gemm_checks.py (`route` for the lone product,
`many_splits` for the pair and the group) and from the layouts:
    lone product    [splits M N fp32 slabs] [column-sum scratch at the next multiple of 256 B]; the scratch is
                    [splits][M] fp32 on the 256 x 256 kernel and the column-sum pass's own workspace
                    (ssl4gie_colsum_workspace_bytes, norm.hip: not under test here) on the 128-tile kernel;
    pair, group     [slabs of product 0 .. n-1] [[splits][M] column-sum partials of the products with colsum_a], each
                    rounded up to 256 B, and nothing at all when splits == 1;
    fallback        (mixed K, a product the 256 x 256 kernel does not take, a pair with alpha != 1 or unequal accumulate)
                    the products run one by one in the same workspace: the largest lone count.
A split count above 1 can be read back from the byte count, so this pins all three policies."""
import ctypes as C

import pytest

import gemm_checks as gc
from gemm_checks import BF, F32, NONE, spec
from ssl4gie_amd import _lib, ops

CUS = (240, 64, 8)


@pytest.fixture(autouse=True)
def _restore_cus():
    yield
    _lib.load().ssl4gie_set_compute_cus(240)


def tn(M, N, K, colsum=False, alpha=1.0, acc=False):
    return spec(M, N, K, "tn", BF, F32, NONE, alpha, acc=acc, colsum=colsum)


def fill(d, s):
    """a TN descriptor over made-up, 16-byte aligned addresses: the queries read no memory"""
    t = ops._desc(s["M"], s["N"], s["K"], ops.code(s["ab"]), ops.code(s["c"]))
    C.memmove(C.byref(d), C.byref(t), C.sizeof(t))
    d.A, d.sAm, d.sAk = 0x10000, 1, s["M"] + 8
    d.B, d.sBk, d.sBn = 0x20000, s["N"] + 8, 1
    d.C, d.ldc = 0x30000, gc.ldc_of(s)
    d.alpha, d.accumulate = s["alpha"], int(s["acc"])
    if s["colsum"]:
        d.colsum_a = 0x40000


def descs_of(specs):
    descs = (_lib.GemmDesc * len(specs))()
    for d, s in zip(descs, specs):
        fill(d, s)
    return descs


def al256(v):
    return (v + 255) & ~255


def lone_bytes(L, s, cus):
    r = gc.route(s, cus)
    assert r["kind"] in ("tn256", "tn128"), r
    M, N, sp = s["M"], s["N"], r["splits"]
    slabs = sp * M * N * 4 if sp > 1 else 0
    if not s["colsum"]:
        return slabs
    cs = (sp * M * 4 if sp > 1 else 0) if r["kind"] == "tn256" else L.ssl4gie_colsum_workspace_bytes(s["K"], M)
    return al256(slabs) + cs if cs else slabs


def many_bytes(L, specs, cus, entry):
    ok = all(gc.route(s, cus)["kind"] == "tn256" and s["K"] == specs[0]["K"] for s in specs)
    if entry == "pair":
        ok = ok and specs[0]["acc"] == specs[1]["acc"] and all(s["alpha"] == 1.0 for s in specs)
    if not ok:
        return max(lone_bytes(L, s, cus) for s in specs)
    sp = gc.many_splits([{"spec": s} for s in specs], cus, entry)
    if sp == 1:
        return 0
    return (sum(al256(sp * s["M"] * s["N"] * 4) for s in specs) +
            sum(al256(sp * s["M"] * 4) for s in specs if s["colsum"]))


def colsum_patterns(n):
    """no product, the first only, the last only, every product with colsum_a"""
    pats = {(False,) * n, (True,) + (False,) * (n - 1), (False,) * (n - 1) + (True,), (True,) * n}
    return sorted(pats)


# (M, N) of dW = dY^T X: the ViT-B block at 256 x 197 tokens, the MAE decoder block, the ragged and partial shapes of
# tests/test_gpu_gemm_kernels.py, the deep one-tile pair, and three shapes of the 128-tile kernel
VITB = [(2304, 768), (768, 768), (3072, 768), (768, 3072)]
LONE = ([(m, n, 50432) for m, n in VITB] + [(512, 2048, 12544), (2048, 512, 12544)] +
        [(264, 264, 1024), (72, 1032, 1024), (520, 136, 1024), (272, 248, 1088), (256, 256, 16384)] +
        [(72, 136, 1000), (64, 64, 1024), (256, 64, 802816)])
PAIRS = [[(2304, 768, 50432), (768, 768, 50432)], [(3072, 768, 50432), (768, 3072, 50432)],
         [(512, 2048, 12544), (2048, 512, 12544)],
         [(264, 264, 1024), (72, 1032, 1024)], [(72, 1032, 1024), (520, 136, 1024)], [(520, 136, 1024), (264, 264, 1024)],
         [(256, 256, 16384), (256, 256, 16384)],
         [(264, 264, 1024), (256, 256, 2048)],        # mixed K: fallback
         [(64, 64, 1024), (264, 264, 1024)],          # M N < 65536: fallback
         [(256, 64, 802816), (72, 136, 1000)]]        # two 128-tile products: fallback
GROUPS = PAIRS + [[(m, n, 50432) for m, n in VITB], [(2304, 768, 50432)], [(256, 256, 16384)],
                  [(264, 264, 1024), (72, 1032, 1024), (520, 136, 1024)],
                  [(m, n, 50432) for m, n in VITB[:3]] + [(64, 64, 50432)]]   # one product too small: fallback


@pytest.mark.parametrize("cus", CUS)
def test_lone_workspace(cus):
    L = _lib.load()
    assert L.ssl4gie_set_compute_cus(cus) == 0
    kinds = set()
    for M, N, K in LONE:
        for colsum in (False, True):
            s = tn(M, N, K, colsum)
            kinds.add(gc.route(s, cus)["kind"])
            got = L.ssl4gie_gemm_workspace_bytes(descs_of([s]))
            assert got == lone_bytes(L, s, cus), (gc.describe(s), cus, got)
    assert kinds == {"tn256", "tn128"}


@pytest.mark.parametrize("cus", CUS)
def test_pair_workspace(cus):
    L = _lib.load()
    assert L.ssl4gie_set_compute_cus(cus) == 0
    variants = [dict(), dict(acc=(True, True)), dict(acc=(True, False)), dict(alpha=(1.0, 0.5))]
    for shapes in PAIRS:
        for v in variants:
            for pat in colsum_patterns(2):
                specs = [tn(m, n, k, c, v.get("alpha", (1.0, 1.0))[i], v.get("acc", (False, False))[i])
                         for i, ((m, n, k), c) in enumerate(zip(shapes, pat))]
                d = descs_of(specs)
                got = L.ssl4gie_gemm_tn_pair_workspace_bytes(C.byref(d[0]), C.byref(d[1]))
                assert got == many_bytes(L, specs, cus, "pair"), ([gc.describe(s) for s in specs], cus, got)


@pytest.mark.parametrize("cus", CUS)
def test_group_workspace(cus):
    L = _lib.load()
    assert L.ssl4gie_set_compute_cus(cus) == 0
    for shapes in GROUPS:
        for alpha, acc in ((1.0, False), (0.5, True)):      # the group takes any alpha and accumulate per product
            for pat in colsum_patterns(len(shapes)):
                specs = [tn(m, n, k, c, alpha if i == 0 else 1.0, acc and i % 2 == 0)
                         for i, ((m, n, k), c) in enumerate(zip(shapes, pat))]
                got = L.ssl4gie_gemm_tn_group_workspace_bytes(descs_of(specs), len(specs))
                assert got == many_bytes(L, specs, cus, "group"), ([gc.describe(s) for s in specs], cus, got)


def test_the_three_policies_show_in_the_byte_counts():
    """two 256 x 256 products over K = 16384 at 240 CUs: 32 splits as a pair (90 wanted) and as a group (120 wanted);
    one of them alone wants 180 and also stops at 16384 / 64 / 8 = 32; over K = 50432 the lone cap of 256 does not
    bind (180 of 98 possible), the pair's and the group's 64 do"""
    L = _lib.load()
    assert L.ssl4gie_set_compute_cus(240) == 0
    slab = 256 * 256 * 4
    two = [tn(256, 256, 16384), tn(256, 256, 16384, True)]
    d = descs_of(two)
    assert L.ssl4gie_gemm_tn_pair_workspace_bytes(C.byref(d[0]), C.byref(d[1])) == 2 * 32 * slab + 32 * 256 * 4
    assert L.ssl4gie_gemm_tn_group_workspace_bytes(d, 2) == 2 * 32 * slab + 32 * 256 * 4
    assert L.ssl4gie_gemm_workspace_bytes(C.byref(d[0])) == 32 * slab
    deep = [tn(256, 256, 50432), tn(256, 256, 50432)]
    d = descs_of(deep)
    assert L.ssl4gie_gemm_workspace_bytes(C.byref(d[0])) == 98 * slab
    assert L.ssl4gie_gemm_tn_pair_workspace_bytes(C.byref(d[0]), C.byref(d[1])) == 2 * 64 * slab
    assert L.ssl4gie_gemm_tn_group_workspace_bytes(d, 2) == 2 * 64 * slab
