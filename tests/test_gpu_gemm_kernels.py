"""Every GEMM kernel, split plan and epilogue of gemm.hip, gemm_nt256.hip, gemm_tn256.hip and gemm256.h against a plain
fp64 reference, per element (tests/gemm_checks.py: the reference, the bounds, how their constants were derived, the
input families and the case list; tests/test_gemm_checks_cpu.py: proof that the checks bite).  Through `ops._desc` and
the C ABI directly (ssl4gie_gemm, ssl4gie_gemm_tn_pair, ssl4gie_gemm_tn_group), so that strides, alpha and the guard
bands are the test's: every output lies in a sentinel-filled buffer with ldc > N, every operand between NaN bands with
lda > K, ldb > K and ldr != ldc (fp32 C also with ldc = 4 mod 8), and the split-K workspace is handed over full of NaN.  No environment knob is used;
the only runtime handle is ssl4gie_set_compute_cus, restored to 240 after every case and by a module fixture.

Case list (gemm_checks.gpu_*_specs): the generic kernel in all four type pairs and layouts, M, N in {1 .. 130}, K in
{0 .. 100}, epilogues 0..6, alpha, accumulate, colsum_a, two-level batches; the 128 x 128 NT kernel (bf16 and fp32 C,
epilogues 0..6, ragged M and N, a multi-round walk with one K-tile per tile); the 256-wide NT kernels forced by the
column statistics, EPI_ADD_AUX and EPI_AFFINE_AUX_RELU (nj = 2, 3, 4; C == NULL) and reached through the heuristic
(ragged and full 16383.. x 128..768 products: streaming stores, the table and polynomial GELU); the 128-tile TN kernel
with 1 .. 256 slabs and the three slab reductions; the 256 x 256 TN kernels (k-split and partial) at four CU counts; the
pair and the group (whole-K route, split route, fallbacks); grid independence; the refusals of the interface.

Variants reached, from one `rocprofv3 --kernel-trace --stats` run of this module in a run of its own (79 distinct
GEMM / reduction kernels; `route` labels every case and the last test prints the counts per label):
    gemm_generic_kernel<TAB, TC>            all four: <f32,f32> <f32,bf16> <bf16,f32> <bf16,bf16>
    gemm_bf16_nt_kernel<TC, MODE>           all fourteen: TC in {f32, bf16} x MODE 0..6
    gemm_bf16_nt256_kernel<TC, MODE, CONV=0, STATS, NJ, NTS (streaming), TAB (table)>
        f32,  MODE 0 / 1 / 3          NJ 3, 4            NTS false and true
        bf16, MODE 0 / 1              NJ 3, 4            NTS false and true;   NJ 2: NTS true only (*)
        bf16, MODE 2 / 5              NJ 3 (polynomial)  NTS false and true;   NJ 4: TAB, NTS false and true (**)
        bf16, MODE 4 / 6              NJ 3, 4            NTS false and true
        bf16, MODE 8 / 9              NJ 2, 3, 4         NTS false and true
        bf16, MODE 0, STATS           NJ 2, 3, 4         (no streaming twin exists)
    gemm_bf16_tn_kernel; slab_reduce_kernel, slab_reduce_wide_kernel<4>, <16>
    gemm_bf16_tn256k_kernel<CS>             CS false and true (lone products, pair, group)
    gemm_bf16_tn256_kernel<CS, 0, PART=true>  CS false and true (the partial kernel)
  Reachable in the default environment and not reached: none.  Every GEMM kernel the library holds is reached here or,
  for CONV 1 / 2 and MODE 7 (the implicit-convolution operand), in tests/test_gpu_conv.py, with one exception:
    (**) MODE 2 / 5 on NJ 4 in the polynomial form, which the supported switch SSL4GIE_GELU_TABLE=0 (README.md) selects.
  Kernels that used to sit behind A/B knobs no longer exist (profiles/HISTORY.md, "Retired knobs"):
    (*)  bf16 MODE 0 / 1 on NJ 2 has the streaming-store form only: the heuristic wants 128 tiles, one column tile means
         M >= 32513, and streaming starts at M = 16384 (nt256_exists in gemm_nt256.hip states it);
    column-split: gemm_bf16_tn256_kernel<CS, 0, PART=false> is gone, full tiles of plain operands always take the k-split
    kernel; so are the loader-wave and four-phase forms of the NT kernel and the five-stage ring of the k-split TN
    kernel, which a debug build of the library used to hold.
  FULL is no instantiation of its own: gemm256.h takes the full / ragged epilogue per tile at run time, so every ragged
  shape with more than one tile runs both; the full-tile twins (16384, 32768 rows) run the full one alone.
  The 256 x 256 TN kernels take a product only from M N >= 65536 (and K >= 1024) on: the partial kernel's lone shape is
  272 x 248 x 1088 (17 K-tiles split 8 / 9) and the pair's ragged products are 264 x 264, 72 x 1032 and 520 x 136 at
  K = 1024; 264 x 136, 72 x 520 and 64 x 64 are below the rule and run as the pair's fallback on the 128-tile kernel.
  512 x 768 and 520 x 600 at K = 1024 have six and nine tiles: whole-K (splits == 1) at 8 CUs, two splits otherwise.
  Across tile widths (8 CUs: 256-wide, 64 / 240 CUs: 192-wide tiles) the bits agreed as well on the MI355X.

Run time on an MI355X: about 14 s for the 64 tests, the slowest 1.0 s (tests/test_gpu_attention_kernels.py: 10 s)."""
import ctypes as C
from collections import Counter

import pytest
import torch

import gemm_checks as gc
from gemm_checks import ADD_AUX, AFFINE, BF, BIAS, BIAS_GELU, BIAS_GELU_GRAD, BIAS_RESIDUAL, DGELU, F32, MUL_AUX, NONE, spec

pytestmark = pytest.mark.gpu
DEV = "cuda"
EARG = 1000
WORST = {}      # worst error / (2^-24 mag) per check and class over the module (printed by the last test)
LABELS = Counter()


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from ssl4gie_amd import _lib
    L = _lib.load()
    yield
    L.ssl4gie_set_compute_cus(240)


def done(rep):
    for n, v in rep.worst.items():
        WORST[n] = max(WORST.get(n, 0.0), v)
    rep.assert_ok()


class Cus:
    """ssl4gie_set_compute_cus(n) for the body, 240 afterwards whatever happens"""

    def __init__(self, n):
        self.n = n

    def __enter__(self):
        from ssl4gie_amd import _lib
        assert _lib.load().ssl4gie_set_compute_cus(self.n) == 0

    def __exit__(self, *a):
        from ssl4gie_amd import _lib
        _lib.load().ssl4gie_set_compute_cus(240)


def build(case):
    """the case's windows on the device and the descriptor that points into them"""
    from ssl4gie_amd import ops
    s, w = case["spec"], case["win"]
    bufs = {n: w[n].buf.to(DEV) for n in w}
    P = lambda n: bufs[n].data_ptr() + w[n].off * bufs[n].element_size()
    d = ops._desc(s["M"], s["N"], s["K"], ops.code(s["ab"]), ops.code(s["c"]))
    d.batch1, d.batch2 = s["batch"]
    d.A = P("A")
    d.sAb1, d.sAb2, d.sAm, d.sAk = w["A"].strides
    d.B = P("B")
    d.sBb1, d.sBb2, d.sBk, d.sBn = w["B"].strides
    d.C = None if s["c_null"] else P("C")
    d.ldc = case["ldc"]
    d.sCb1, d.sCb2 = w["C"].strides[:2]
    d.alpha, d.epilogue, d.accumulate = s["alpha"], s["epi"], int(s["acc"])
    epi = s["epi"]
    if epi == AFFINE or (s["bias"] and epi in (BIAS, BIAS_GELU, BIAS_RESIDUAL, BIAS_GELU_GRAD)):
        d.bias = P("bias")
    if epi == BIAS_RESIDUAL:
        d.residual, d.ldr = P("residual"), case["ldr"]
    if epi in (DGELU, MUL_AUX, ADD_AUX) or (epi == AFFINE and s["aux"]):
        d.aux = P("aux")
    if epi in (BIAS_GELU, BIAS_GELU_GRAD):
        d.out2 = P("out2")
    if epi == AFFINE:
        d.scale, d.relu = P("scale"), int(s["relu"])
    if s["colsum"]:
        d.colsum_a = P("colsum")
    if s["colstats"]:
        d.colstats = P("colstats")
    return d, bufs


def nan_workspace(nbytes):
    return torch.full((nbytes // 4 + 16,), float("nan"), dtype=F32, device=DEV)


def launch(case, cus=None, short=0):
    """-> (return code, the four output buffers on the device, every buffer of the case on the device)"""
    from ssl4gie_amd import _lib, ops
    L = _lib.load()
    d, bufs = build(case)
    with Cus(cus or case["spec"]["cus"]):
        n = L.ssl4gie_gemm_workspace_bytes(C.byref(d))
        ws = nan_workspace(n)
        rc = L.ssl4gie_gemm(C.byref(d), ops.ptr(ws), max(n - short, 0), ops.stream())
        torch.cuda.synchronize()
    return rc, {k: bufs[k] for k in ("C", "out2", "colsum", "colstats")}, bufs


def judge(case, outs, cus=None, tag=None):
    """the checks of one case: where the operands live (the device from 1e8 multiply-adds on)"""
    s = case["spec"]
    r = gc.route(s, cus)
    LABELS[gc.route_label(r)] += 1
    if gc.macs(s) > gc.BIG_MACS:
        case = gc.to_device(case, DEV)
    else:
        outs = {k: v.cpu() for k, v in outs.items()}
    return gc.check_case(case, outs, r["splits"], r["gelu"], tag=tag, generic=r["kind"] == "generic")


def run_spec(s, rep, cus=None):
    case = gc.make_case(s)
    rc, outs, _ = launch(case, cus)
    assert rc == 0, (rc, gc.describe(s))
    rep.merge(judge(case, outs, cus))
    return case, outs


SPECS = list(gc.gpu_specs())


@pytest.mark.parametrize("group", gc.groups(SPECS))
def test_gemm(group):
    """every case of the group: per-element bounds, exact families bit for bit, sentinels, NaN bands; a product with
    column statistics is run a second time with C == NULL: the same statistics, bit for bit"""
    rep = gc.Report()
    for g, s in SPECS:
        if g != group:
            continue
        case, outs = run_spec(s, rep)
        if s["colstats"]:
            s2 = dict(s, c_null=True)
            case2 = gc.make_case(s2)
            rc, outs2, _ = launch(case2)
            assert rc == 0, gc.describe(s2)
            rep.merge(judge(case2, outs2))
            rep.same("colstats", outs2["colstats"], outs["colstats"], "C == NULL gives other statistics")
    done(rep)


# ===================================================================== pair and group
def launch_many(cases, entry, cus=240):
    from ssl4gie_amd import _lib, ops
    L = _lib.load()
    n = len(cases)
    descs = (_lib.GemmDesc * n)()
    keep = []
    for i, c in enumerate(cases):
        d, bufs = build(c)
        C.memmove(C.byref(descs[i]), C.byref(d), C.sizeof(d))
        keep.append(bufs)
    with Cus(cus):
        if entry == "pair":
            nb = L.ssl4gie_gemm_tn_pair_workspace_bytes(C.byref(descs[0]), C.byref(descs[1]))
            ws = nan_workspace(nb)
            rc = L.ssl4gie_gemm_tn_pair(C.byref(descs[0]), C.byref(descs[1]), ops.ptr(ws), nb, ops.stream())
        else:
            nb = L.ssl4gie_gemm_tn_group_workspace_bytes(descs, n)
            ws = nan_workspace(nb)
            rc = L.ssl4gie_gemm_tn_group(descs, n, ops.ptr(ws), nb, ops.stream())
        torch.cuda.synchronize()
    assert rc == 0, (entry, rc)
    return [{k: b[k] for k in ("C", "out2", "colsum", "colstats")} for b in keep], nb


def judge_many(cases, outs, splits, rep, what):
    for c, o in zip(cases, outs):
        o = {k: v.cpu() for k, v in o.items()}
        rep.merge(gc.check_case(c, o, splits, tag=what + " " + gc.describe(c["spec"])))


def tn(M, N, Kd, fam, alpha=1.0, acc=False, colsum=False, seed=0):
    return gc.make_case(spec(M, N, Kd, "tn", BF, F32, NONE, alpha, acc=acc, colsum=colsum, family=fam, seed=seed))


def deep_two(family):
    """two one-tile products over K = 16384: 32 splits at 240 CUs in the pair and in the group, the count from which a
    lone product without column sums takes the wide reduction; the second product carries colsum_a"""
    return [tn(256, 256, 16384, family, seed=11), tn(256, 256, 16384, family, colsum=True, seed=12)]


@pytest.mark.parametrize("family", ["gauss", "integers", "cancel"])
def test_tn_pair(family):
    """ragged products of one launch (alpha = 1: the pair's rule), with and without the fused column sums and
    accumulate; at 8 CUs the split count changes; two one-tile products over K = 16384: 32 slabs each"""
    rep = gc.Report()
    shapes = ((264, 264), (72, 1032), (520, 136))      # each M N >= 65536: the 256 x 256 kernel's own rule
    for cus in (240, 8):
        for i in range(3):
            (m0, n0), (m1, n1) = shapes[i], shapes[(i + 1) % 3]
            acc = i == 1
            cases = [tn(m0, n0, 1024, family, acc=acc, colsum=i != 2, seed=i), tn(m1, n1, 1024, family, acc=acc, colsum=i == 0, seed=i + 5)]
            outs, _ = launch_many(cases, "pair", cus)
            judge_many(cases, outs, gc.many_splits(cases, cus, "pair"), rep, "pair cus %d" % cus)
    cases = deep_two(family)
    assert gc.many_splits(cases, 240, "pair") == 32
    outs, _ = launch_many(cases, "pair", 240)
    judge_many(cases, outs, 32, rep, "pair deep")
    done(rep)


@pytest.mark.parametrize("family", ["gauss", "integers", "cancel"])
def test_tn_group(family):
    """three two-tile products at 8 CUs: six whole-K tiles, no slabs (the workspace query says 0 bytes), with alpha,
    accumulate and colsum_a per product; the same group at 240 CUs splits K; one product alone; two one-tile products
    over K = 16384: 32 slabs each"""
    rep = gc.Report()
    mk = lambda: [tn(512, 256, 1024, family, 0.5, True, True, 1), tn(256, 264, 1024, family, -2.0, False, True, 2),
                  tn(264, 256, 1024, family, 1.0, True, False, 3)]
    cases = mk()
    outs, nb = launch_many(cases, "group", 8)
    assert nb == 0, nb
    judge_many(cases, outs, 1, rep, "group whole-K")
    cases = mk()
    outs, nb = launch_many(cases, "group", 240)
    assert nb > 0
    assert gc.many_splits(cases, 240, "group") == max(1, min((240 + 3) // 6, 1024 // 64 // 8, 64))
    judge_many(cases, outs, gc.many_splits(cases, 240, "group"), rep, "group split")
    cases = mk()[:1]
    outs, nb = launch_many(cases, "group", 64)
    assert gc.many_splits(cases, 64, "group") == max(1, min((64 + 1) // 2, 2, 64))
    judge_many(cases, outs, gc.many_splits(cases, 64, "group"), rep, "group of one")
    cases = deep_two(family)
    assert gc.many_splits(cases, 240, "group") == 32
    outs, nb = launch_many(cases, "group", 240)
    assert nb == 2 * 32 * 256 * 256 * 4 + 32 * 256 * 4, nb
    judge_many(cases, outs, 32, rep, "group deep")
    done(rep)


@pytest.mark.parametrize("entry", ["pair", "group"])
def test_tn_pair_and_group_fall_back(entry):
    """K % 64 != 0, mixed K, products too small for the 256 x 256 kernel, alpha != 1 in a pair: the products run one
    by one, each within its own bounds"""
    rep = gc.Report()
    for cases in ([tn(264, 136, 1000, "gauss", 0.5, True, True), tn(72, 520, 1000, "integers", 1.0, False, True)],
                  [tn(264, 264, 1024, "integers", 1.0, False, True), tn(256, 256, 2048, "gauss", 1.0, True, False)],
                  [tn(264, 136, 1024, "gauss", 1.0, False, True), tn(72, 520, 1024, "integers", 1.0, False, True)],
                  [tn(64, 64, 1024, "gauss", 1.0, True, False), tn(264, 264, 1024, "cancel", 1.0, True, False)],
                  [tn(264, 256, 1088, "gauss", 0.5, False, True), tn(256, 256, 1088, "integers", -2.0, True, True)]):
        if entry == "group" and cases[0]["spec"]["K"] == 1088:
            continue                                    # the group takes alpha != 1: no fallback
        outs, _ = launch_many(cases, entry)
        for c, o in zip(cases, outs):
            rep.merge(judge(c, o, tag=entry + " fallback " + gc.describe(c["spec"])))
    done(rep)


# ===================================================================== grid independence
def test_nt128_grid_independence():
    """one route (128 x 128 tiles), 25 tiles on 16, 128 and 480 workgroups: the same bits for every epilogue"""
    rep = gc.Report()
    for ct in (BF, F32):
        for epi in range(7):
            s = spec(640, 640, 128, "nt", BF, ct, epi, 0.75, family="gauss", seed=epi)
            case = gc.make_case(s)
            ref = None
            for cus in (240, 8, 64):
                rc, outs, _ = launch(case, cus)
                assert rc == 0
                if ref is None:
                    ref = outs
                    rep.merge(judge(case, outs, cus))
                else:
                    for n in ("C", "out2"):
                        rep.same(n, outs[n], ref[n], "cus %d: not the bits of cus 240 (%s)" % (cus, gc.describe(s)))
    done(rep)


def test_nt256_grid_independence():
    """the 256-wide kernels: 64 and 240 CUs choose the same tile width (192): the same bits; 8 CUs choose 256-wide
    tiles: within the bounds.  Whether the bits agree across the widths as well is printed (the accumulation order per
    element is the same; on an MI355X they did)"""
    rep = gc.Report()
    agree = True
    for i, (epi, stats, _, relu, aux) in enumerate(gc._forced_variants(0)):
        s = spec(1500, 512, 192, "nt", BF, BF, epi, 0.75, colstats=stats, relu=relu, aux=aux, family="gauss", seed=i)
        assert (gc.route(s, 240)["nj"], gc.route(s, 64)["nj"], gc.route(s, 8)["nj"]) == (3, 3, 4)
        case = gc.make_case(s)
        ref = None
        for cus in (240, 64, 8):
            rc, outs, _ = launch(case, cus)
            assert rc == 0
            rep.merge(judge(case, outs, cus))
            if ref is None:
                ref = outs
            elif cus == 64:
                for n in ("C", "colstats"):
                    rep.same(n, outs[n], ref[n], "cus 64: not the bits of cus 240 (%s)" % gc.describe(s))
            else:
                agree = agree and all(torch.equal(outs[n], ref[n]) for n in ("C", "colstats"))
    print("256-wide and 192-wide tiles give the same bits:", agree)
    done(rep)


# ===================================================================== interface
def test_refused_arguments():
    """what include/ssl4gie_hip.h says is refused: SSL4GIE_EARG, and nothing written"""
    bad = [
        ("ADD_AUX with fp32 C", spec(300, 264, 64, "nt", BF, F32, ADD_AUX)),
        ("AFFINE with fp32 C", spec(300, 264, 64, "nt", BF, F32, AFFINE)),
        ("colstats with a bias epilogue", spec(300, 264, 64, "nt", BF, BF, BIAS, colstats=True)),
        ("colstats with fp32 C", spec(300, 264, 64, "nt", BF, F32, NONE, colstats=True)),
        ("colstats with N % 8 != 0", spec(300, 260, 64, "nt", BF, BF, NONE, colstats=True)),
        ("accumulate with an epilogue", spec(64, 64, 64, "nt", BF, F32, BIAS, acc=True)),
        ("batch > 1 with an epilogue", spec(64, 64, 16, "nn", F32, F32, BIAS, batch=(2, 1))),
        ("colsum_a with sAm != 1", spec(64, 64, 64, "nt", BF, F32, NONE, colsum=True)),
        ("C == NULL without colstats", spec(300, 264, 64, "nt", BF, BF, NONE, c_null=True)),
    ]
    rep = gc.Report()
    for what, s in bad:
        case = gc.make_case(s)
        rc, outs, _ = launch(case)
        assert rc == EARG, (what, rc)
        for n, b in outs.items():
            assert torch.equal(b.cpu(), case["win"][n].buf), (what, n)
    # a TN workspace one byte short (both TN kernels, and the separate column-sum pass of the generic kernel)
    for s in (spec(72, 136, 1000, "tn", BF, F32, NONE), spec(256, 256, 1024, "tn", BF, F32, NONE, colsum=True),
              spec(64, 63, 33, "tn", F32, F32, NONE, colsum=True)):
        case = gc.make_case(s)
        d, _ = build(case)
        from ssl4gie_amd import _lib
        assert _lib.load().ssl4gie_gemm_workspace_bytes(C.byref(d)) > 0, gc.describe(s)
        rc, outs, _ = launch(case, short=1)
        assert rc == EARG, (gc.describe(s), rc)
        for n, b in outs.items():
            assert torch.equal(b.cpu(), case["win"][n].buf), (gc.describe(s), n)
        rc, outs, _ = launch(case)
        assert rc == 0
        rep.merge(judge(case, outs))
    done(rep)


def test_empty_products_write_nothing():
    for M, N in ((0, 64), (64, 0), (0, 0)):
        for layout, ab, ct in (("nt", BF, BF), ("tn", BF, F32), ("nn", F32, F32)):
            s = spec(M, N, 64, layout, ab, ct, NONE)
            case = gc.make_case(s)
            rc, outs, _ = launch(case)
            assert rc == 0, gc.describe(s)
            for n, b in outs.items():
                assert torch.equal(b.cpu(), case["win"][n].buf), (gc.describe(s), n)


def test_report_worst_ratios():
    """the "kernels' worst ratio" column of gemm_checks' table, and the variants the module reached (by label)"""
    for n in gc.CHECKS:
        print("worst %-10s %8.3f   (k = %g)" % (n, WORST.get(n, float("nan")), gc.K[n]))
    for label, cnt in sorted(LABELS.items()):
        print("%5d  %s" % (cnt, label))
    assert set(WORST) <= set(gc.CHECKS)
