"""Every BatchNorm entry point of resnet_ops.hip against a plain fp64 reference (tests/bn_checks.py: the
reference, the per-element / per-channel bounds and how their constants were derived), through ssl4gie_amd.ops.

Two families over one case list that puts a case on every branch boundary of the kernels:
  exact   small-integer operands and handed-in (mean, rstd), so that every term and every partial sum is an
          integer or a dyadic value below 2^24: any summation order is exact and dgamma / dbeta / sums / dres
          must equal the fp64 values bit for bit; statistics of integer maps and of hand-made integer partials
          within 2 ulp of the correctly rounded value (one division, one subtraction);
  real    random maps (gamma with zeros and negatives, channels with |mean| = 8 sigma, a constant channel),
          fp32 and bf16, every relu x residual combination an entry point accepts, under the derived bounds.
Case list: lane folding (C / V a folded power of two, not a power of two, one full strip, a ragged second strip,
many strips) x rows across the 2- and 4-row unrolled loops; 1 ... 1024 partitions on the direct path (32+: the
eight-deep unroll of bn_sum_partials, 257+: the 1024-thread tail), hand-made partial counts up to 25 088 (> 2048:
bn_fold_partials_kernel); the production maps of one 256-image view.  The ids say which branch a case is on."""
import math

import pytest
import torch

import bn_checks as bc

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32, BF, F64 = torch.float32, torch.bfloat16, torch.float64
COMBOS = ((False, False), (True, False), (False, True), (True, True))   # relu, residual


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from ssl4gie_amd import _lib
    _lib.load()


def dn(dtype):
    return "bf16" if dtype == BF else "fp32"


def tail_of(parts):
    """which tail of the statistics / gradient sums `parts` partial rows take"""
    if parts > 2048:
        return "fold%s" % ("" if parts % 256 == 0 else "+rem")
    if parts > 256:
        return "tail1024"
    return "tail256" + ("+unroll8" if parts >= 29 else "")


def pack_bits(mask):
    w = torch.tensor([1, 2, 4, 8, 16, 32, 64, 128], dtype=torch.int32, device=mask.device)
    return (mask.reshape(-1, 8).to(torch.int32) * w).sum(1).to(torch.uint8)


def unpack_bits(bits, rows, C):
    sh = torch.arange(8, dtype=torch.int32, device=bits.device)
    return ((bits.view(-1, 1).to(torch.int32) >> sh) & 1).bool().view(rows, C)


# ===================================================================== real-valued family
def forward(c, how):
    from ssl4gie_amd import ops
    rm, rv = c["rm0"].clone(), c["rv0"].clone()
    a = (c["gamma"], c["beta"], c["res"], rm, rv, c["momentum"], c["eps"])
    bits = None
    if how == "direct":
        y, mean, rstd = ops.bn_fwd(c["x"], *a, c["relu"], True)
    elif how == "partials":
        y, mean, rstd = ops.bn_fwd(c["x"], *a, c["relu"], True, partials=c["partials"])
    else:
        assert how == "bits" and c["relu"]
        y, bits, mean, rstd = ops.bn_fwd_bits(c["x"], *a, c["partials"])
    return {"y": y, "mean": mean, "rstd": rstd, "rm": rm, "rv": rv, "bits": bits}


def check_fwd(rep, c, f, st, tag):
    bc.check_stats(rep, st, c["eps"], f["mean"], None, f["rstd"],
                   (f["rm"], f["rv"], c["rm0"], c["rv0"], c["momentum"]), tag=tag)
    bc.check_forward(rep, c["x"], f["mean"], f["rstd"], c["gamma"], c["beta"], c["res"], c["relu"], f["y"], tag=tag)
    if f["bits"] is not None and not torch.equal(f["bits"], pack_bits(f["y"] > 0)):
        rep.fail(tag + "bits", "the bit map is not y > 0 of the stored output")


def backward_all(rep, c, f, tag, halves=True):
    """every backward entry point that accepts this case, from the forward's stored (y / bits, mean, rstd)"""
    from ssl4gie_amd import ops
    x, dy, y, gamma, mean, rstd = c["x"], c["dy"], f["y"], c["gamma"], f["mean"], f["rstd"]
    relu, res, dt, rows = c["relu"], c["res"] is not None, c["dtype"], c["rows"]
    bw = bc.ref_backward(dy, (y > 0) if relu else None, x, mean, rstd, gamma, 1.0 / rows)
    fresh = lambda: (torch.full_like(c["dg0"], math.nan), torch.full_like(c["db0"], math.nan))
    # one call: overwrite, then accumulate
    dg, db = fresh()
    dx, dres = ops.bn_bwd(dy, y if relu else None, x, gamma, mean, rstd, relu, res, dg, db, False)
    bc.check_backward(rep, bw, dt, dx, dres, None, dg, db, tag=tag + "bn_bwd.")
    dg, db = c["dg0"].clone(), c["db0"].clone()
    dx, dres = ops.bn_bwd(dy, y if relu else None, x, gamma, mean, rstd, relu, not res, dg, db, True)
    bc.check_backward(rep, bw, dt, dx, dres, None, dg, db, c["dg0"], c["db0"], tag=tag + "bn_bwd+acc.")
    del dx, dres
    w = 4       # "global" batch of the SyncBatchNorm halves: w ranks with these rows each
    if halves:
        sums, dres = ops.bn_bwd_reduce(dy, y if relu else None, x, mean, rstd, relu, res)
        bc.check_backward(rep, bw, dt, None, dres, sums, tag=tag + "bn_bwd_reduce.")
        gs = sums * w
        bwg = bc.ref_backward(dy, (y > 0) if relu else None, x, mean, rstd, gamma, 1.0 / (w * rows), gs)
        dx = ops.bn_bwd_apply(dy, y if relu else None, x, gamma, mean, rstd, gs, 1.0 / (w * rows), relu)
        bc.check_backward(rep, bwg, dt, dx, tag=tag + "bn_bwd_apply.")
        del bwg, dx, dres
    if relu and not res:
        for acc in (False, True):
            dg, db = (c["dg0"].clone(), c["db0"].clone()) if acc else fresh()
            dx = ops.bn_bwd_xmask(dy, x, gamma, c["beta"], mean, rstd, dg, db, acc)
            bc.check_backward(rep, bw, dt, dx, None, None, dg, db, c["dg0"] if acc else None,
                              c["db0"] if acc else None, tag=tag + "bn_bwd_xmask%s." % ("+acc" if acc else ""))
        if halves:
            sums = ops.bn_bwd_reduce_xmask(dy, x, gamma, c["beta"], mean, rstd)
            bc.check_backward(rep, bw, dt, sums=sums, tag=tag + "bn_bwd_reduce_xmask.")
            gs = sums * w
            bwg = bc.ref_backward(dy, y > 0, x, mean, rstd, gamma, 1.0 / (w * rows), gs)
            dx = ops.bn_bwd_apply_xmask(dy, x, gamma, c["beta"], mean, rstd, gs, 1.0 / (w * rows))
            bc.check_backward(rep, bwg, dt, dx, tag=tag + "bn_bwd_apply_xmask.")
            del bwg, dx
    if relu and dt == BF:
        bits = f["bits"] if f["bits"] is not None else pack_bits(y > 0)
        for acc in (False, True):
            dg, db = (c["dg0"].clone(), c["db0"].clone()) if acc else fresh()
            dx, dres = ops.bn_bwd_bits(dy, bits, x, gamma, mean, rstd, dg, db, acc)
            bc.check_backward(rep, bw, dt, dx, dres, None, dg, db, c["dg0"] if acc else None,
                              c["db0"] if acc else None, tag=tag + "bn_bwd_bits%s." % ("+acc" if acc else ""))
        if halves:
            sums, dres = ops.bn_bwd_reduce_bits(dy, bits, x, mean, rstd)
            bc.check_backward(rep, bw, dt, None, dres, sums, tag=tag + "bn_bwd_reduce_bits.")
            gs = sums * w   # second half: bn_bwd_apply on the masked gradient, relu 0
            bwg = bc.ref_backward(dy, y > 0, x, mean, rstd, gamma, 1.0 / (w * rows), gs)
            dx = ops.bn_bwd_apply(dres, None, x, gamma, mean, rstd, gs, 1.0 / (w * rows), False)
            bc.check_backward(rep, bwg, dt, dx, tag=tag + "bn_bwd_reduce_bits+apply.")


def coef_checks(rep, c, f, st, tag):
    """eval-mode forward and the coefficient entry points, on the statistics the training forward returned"""
    from ssl4gie_amd import ops
    mean, rstd, gamma, beta = f["mean"], f["rstd"], c["gamma"], c["beta"]
    y, _, _ = ops.bn_fwd(c["x"], gamma, beta, c["res"], None, None, 0.0, c["eps"], c["relu"], False, mean=mean,
                         rstd=rstd)
    bc.check_forward(rep, c["x"], mean, rstd, gamma, beta, c["res"], c["relu"], y, tag=tag + "eval.")

    def coef_ok(coef, mean, rstd, name):
        a = rstd.to(F64) * (1.0 if gamma is None else gamma.to(F64))
        b0 = 0.0 if beta is None else beta.to(F64)
        rep.ratio(tag + name + ".a", coef[0], a, a.abs(), kname="y")
        rep.ratio(tag + name + ".b", coef[1], b0 - mean.to(F64) * a, abs(b0) + (mean.to(F64) * a).abs(), kname="y")
    coef_ok(ops.bn_coef_stats(mean, rstd, gamma, beta), mean, rstd, "bn_coef_stats")
    if "partials" in c:
        rm, rv = c["rm0"].clone(), c["rv0"].clone()
        coef, m2, r2 = ops.bn_coef_partials(c["partials"], c["rows"], gamma, beta, rm, rv, c["momentum"], c["eps"])
        bc.check_stats(rep, st, c["eps"], m2, None, r2, (rm, rv, c["rm0"], c["rv0"], c["momentum"]),
                       tag=tag + "bn_coef_partials.")
        coef_ok(coef, m2, r2, "bn_coef_partials")
        m3, v3 = ops.bn_stats(c["x"], partials=c["partials"])
        bc.check_stats(rep, st, c["eps"], m3, v3, tag=tag + "bn_stats(partials).")


def real_case(rep, c, paths=("direct", "partials", "bits"), halves=True, tag=""):
    """all forward paths of case `c` (already on the device) and every backward behind each"""
    from ssl4gie_amd import ops
    st_p = st_0 = None
    for how in paths:
        if how == "bits" and not (c["relu"] and c["dtype"] == BF):
            continue
        if how != "direct" and "partials" not in c:
            c["partials"] = bc.partials_of(c["x"])
        t = "%s%s." % (tag, how)
        if how == "direct":
            st = st_p = st_p or bc.ref_stats(c["x"], True)
            m, v = ops.bn_stats(c["x"])
            bc.check_stats(rep, st, c["eps"], m, v, tag=t + "bn_stats.")
            if not bool((v[3] == 0).all()):
                rep.fail(t + "bn_stats", "the constant channel's variance is not exactly 0")
        else:
            st = st_0 = st_0 or bc.ref_stats(c["x"], False)
        f = forward(c, how)
        check_fwd(rep, c, f, st, t)
        backward_all(rep, c, f, t, halves and how != "partials")
        if how != "bits":
            coef_checks(rep, c, f, st, t)


def finish(rep):
    worst = {}
    for n, v in rep.worst.items():
        n = n.split(".")[-1].split("[")[0]
        worst[n] = max(worst.get(n, 0.0), v)
    print("worst error / (2^-24 mag):", {n: float("%.3g" % v) for n, v in sorted(worst.items())})
    rep.assert_ok()


@pytest.mark.parametrize("dtype", [F32, BF], ids=dn)
@pytest.mark.parametrize("C", bc.EDGE_C)
def test_real_lane_folding_and_row_edges(C, dtype):
    """C: how the channel groups fold onto a wave; rows: 1, 2, 3 and around m x (rows a lane advances per step),
    m = 1 ... 5 — across the 2-row and 4-row unrolled loops of both reductions and their remainders"""
    rep = bc.Report()
    for rows in bc.edge_rows(C, dtype):
        for relu, res in COMBOS:
            if relu and rows == 1:      # undecidable signs: see bn_checks
                continue
            for affine in ((True, False) if not (relu or res) else (True,)):
                c = bc.to_device(bc.edge_case(rows, C, dtype, relu, res, affine), DEV)
                rep.tag = "rows=%d relu=%d res=%d affine=%d" % (rows, relu, res, affine)
                real_case(rep, c, tag="")
    finish(rep)


@pytest.mark.parametrize("dtype", [F32, BF], ids=dn)
@pytest.mark.parametrize("rows,C,parts", bc.PARTITION_SHAPES,
                         ids=["%dparts-%s" % (p, tail_of(p)) for _, _, p in bc.PARTITION_SHAPES])
def test_real_direct_path_partitions(rows, C, parts, dtype):
    """the direct path's own partials (one partition per 64 Ki elements), forward and backward tails"""
    assert bc.bn_parts(rows, C) == parts
    rep = bc.Report()
    for relu, res in ((True, True), (True, False), (False, False)):
        c = bc.make_case(rows, C, dtype, DEV, 31 * rows + C, relu, res, True)
        rep.tag = "relu=%d res=%d" % (relu, res)
        real_case(rep, c, paths=("direct",))
        del c
    finish(rep)


@pytest.mark.parametrize("parts", bc.PARTIAL_COUNTS, ids=["%dpartials-%s" % (p, tail_of(p)) for p in bc.PARTIAL_COUNTS])
def test_real_statistics_from_partials(parts):
    """hand-made 128-row partials (sums about 0, each correctly rounded from fp64) of a bf16 map into every
    statistics-from-partials entry point; the bounds carry the (1 + mean^2 / var) factor of the unpivoted sums"""
    C = 200 if parts <= 2049 else 64     # 200: the tail's last block of 64 channels is ragged
    rows = parts * 128 - (3 if parts > 1 else 0)
    rep = bc.Report()
    for relu, res in ((True, True), (False, False)):
        c = bc.make_case(rows, C, BF, DEV, 17 * parts, relu, res, True)
        c["partials"] = bc.partials_of(c["x"])
        assert c["partials"].shape[0] == parts
        rep.tag = "relu=%d res=%d" % (relu, res)
        real_case(rep, c, paths=("partials", "bits"), halves=False)
        del c
    finish(rep)


@pytest.mark.parametrize("rows,C,affine", bc.PRODUCTION,
                         ids=["%dx%d-%s" % (r, C, tail_of(bc.bn_parts(r, C))) for r, C, _ in bc.PRODUCTION])
def test_real_production_maps_bf16(rows, C, affine):
    """the maps of one 256-image view, whole (every element, every channel sum, every statistic): direct and
    128-row-partials forward, every backward entry point"""
    rep = bc.Report()
    for relu, res in (((True, True), (True, False)) if affine else ((False, False),)):
        c = bc.make_case(rows, C, BF, DEV, rows + C, relu, res, affine)
        rep.tag = "relu=%d res=%d" % (relu, res)
        real_case(rep, c, halves=rows * C < (1 << 27))
        del c
        torch.cuda.empty_cache()
    finish(rep)


def test_rows_1_running_variance_convention():
    """one row (torch refuses it): variance 0, rstd = eps^-1/2, y = beta + res within the bound, and the unbiased
    factor n / (n - 1) taken as 1 — the running variance is blended with the biased value, 0"""
    from ssl4gie_amd import ops
    for dtype in (F32, BF):
        c = bc.to_device(bc.make_case(1, 64, dtype, "cpu", 3, False, True, True), DEV)
        f = forward(c, "direct")
        rep = bc.Report()
        check_fwd(rep, c, f, bc.ref_stats(c["x"], True), "")
        rep.assert_ok()
        _, var = ops.bn_stats(c["x"])
        assert torch.equal(var, torch.zeros_like(var)) and torch.equal(f["mean"], c["x"][0].float())
        assert torch.allclose(f["rstd"], torch.full_like(var, 1e-5 ** -0.5), rtol=1e-6, atol=0)
        assert torch.allclose(f["rv"], 0.9 * c["rv0"], rtol=1e-6, atol=0)
        bw_rep = bc.Report()
        backward_all(bw_rep, c, f, "")
        bw_rep.assert_ok()


# ===================================================================== exact-integer family
def ulp32(v):
    a = v.abs().float()
    return (torch.nextafter(a, torch.full_like(a, math.inf)) - a).to(F64)


def ints(g, shape, lo, hi, dtype):
    return torch.randint(lo, hi + 1, shape, generator=g, device=DEV).to(dtype)


def pick(g, values, n):
    v = torch.tensor(values, dtype=F32, device=DEV)
    return v[torch.randint(0, len(values), (n,), generator=g, device=DEV)]


def exact_inputs(rows, C, dtype, seed):
    g = torch.Generator(DEV).manual_seed(seed)
    r = 4 if rows <= 4096 else 1       # wider ranges at small shapes
    e = {"x": ints(g, (rows, C), -r, r, dtype), "dy": ints(g, (rows, C), -r, r, dtype),
         "mean": pick(g, [-1.0, 0.0, 1.0], C), "rstd": pick(g, [0.5, 1.0, 2.0], C),
         "gamma": pick(g, [-2.0, -1.0, 0.0, 1.0, 2.0, 3.0], C), "beta": pick(g, [-1.0, 0.0, 1.0], C),
         "y": pick(g, [-1.0, -0.0, 0.0, 1.0, 2.0], rows * C).view(rows, C).to(dtype),   # drawn independently of x
         "dg0": ints(g, (C,), -8, 8, F32), "db0": ints(g, (C,), -8, 8, F32)}
    e["bits"] = torch.randint(0, 256, (rows * C // 8,), generator=g, device=DEV).to(torch.uint8)
    return e


def exact_sums(e, mask):
    """fp64 (g, sum g, sum g xhat), with the proof that any fp32 summation order is exact"""
    g = e["dy"].to(F64)
    if mask is not None:
        g = torch.where(mask, g, torch.zeros_like(g))
    gx = g * ((e["x"].to(F64) - e["mean"].to(F64)) * e["rstd"].to(F64))
    # terms are multiples of 1/2: a partial sum is exact while 2 sum|term| < 2^24
    assert float(g.abs().sum(0).max()) < 2 ** 24 and 2 * float(gx.abs().sum(0).max()) < 2 ** 24
    return g, g.sum(0), gx.sum(0)


def exact_backward(rows, C, dtype, seed):
    from ssl4gie_amd import ops
    e = exact_inputs(rows, C, dtype, seed)
    x, dy, mean, rstd, gamma, beta = e["x"], e["dy"], e["mean"], e["rstd"], e["gamma"], e["beta"]
    a = rstd.to(F64) * gamma.to(F64)
    masks = {"y": e["y"] > 0, "x": x.to(F64) * a + (beta.to(F64) - mean.to(F64) * a) > 0, None: None}
    if dtype == BF:
        masks["bits"] = unpack_bits(e["bits"], rows, C)
    bad = []

    def same(name, got, ref):
        if not torch.equal(got.to(F64), ref):
            bad.append("%s: %d of %d values differ, worst |diff| %g" % (name, int((got.to(F64) != ref).sum()),
                                                                       ref.numel(), float((got.to(F64) - ref).abs().max())))
    for how, mask in masks.items():
        g, s1, s2 = exact_sums(e, mask)
        for acc in (False, True):
            dg, db = (e["dg0"].clone(), e["db0"].clone()) if acc else (torch.full_like(e["dg0"], math.nan),) * 2
            if not acc:
                db = dg.clone()
            dres = None
            if how == "y" or how is None:
                _, dres = ops.bn_bwd(dy, e["y"] if how else None, x, gamma, mean, rstd, how is not None, True, dg, db, acc)
            elif how == "x":
                ops.bn_bwd_xmask(dy, x, gamma, beta, mean, rstd, dg, db, acc)
            else:
                _, dres = ops.bn_bwd_bits(dy, e["bits"], x, gamma, mean, rstd, dg, db, acc)
            t = "mask=%s acc=%d " % (how, acc)
            same(t + "dbeta", db, s1 + (e["db0"].to(F64) if acc else 0))
            same(t + "dgamma", dg, s2 + (e["dg0"].to(F64) if acc else 0))
            if dres is not None:
                same(t + "dres", dres, g)
        if how == "y" or how is None:
            sums, dres = ops.bn_bwd_reduce(dy, e["y"] if how else None, x, mean, rstd, how is not None, True)
            same("bn_bwd_reduce(mask=%s) dres" % how, dres, g)
        elif how == "x":
            sums = ops.bn_bwd_reduce_xmask(dy, x, gamma, beta, mean, rstd)
        else:
            sums, dres = ops.bn_bwd_reduce_bits(dy, e["bits"], x, mean, rstd)
            same("bn_bwd_reduce_bits dres", dres, g)
        same("bn_bwd_reduce(mask=%s) sums" % how, sums, torch.stack([s1, s2]))
    return bad


def exact_statistics(rows, C, dtype, seed):
    """bn_stats / bn_fwd over an integer map: the pivoted sums S, Q are integers, so mean = x0 + fl(S / n) and
    var = fl(fl(Q / n) - fl(d d)), d = fl(S / n): within 2 ulp (of the larger term) of the correctly rounded
    value, plus 2^-23 d^2 — the pivot is a random row, so d^2 is not small against Q / n and the rounding of d
    itself, doubled by the square, has to be counted beside the division and the subtraction; equal to the
    correctly rounded value when n is a power of two and S^2 < 2^24 (every intermediate exact)"""
    from ssl4gie_amd import ops
    e = exact_inputs(rows, C, dtype, seed)
    x = e["x"]
    d = x.to(F64) - x[0].to(F64)
    S, Q, n = d.sum(0), (d * d).sum(0), float(rows)
    assert float(Q.max()) < 2 ** 24 and float(d.abs().sum(0).max()) < 2 ** 24
    m_ref, v_ref = x[0].to(F64) + S / n, Q / n - (S / n) ** 2
    exact = rows & (rows - 1) == 0 and float(S.abs().max()) ** 2 < 2 ** 24
    tol_m = 0 if exact else 2 * ulp32(torch.maximum((S / n).abs(), m_ref.abs()))
    tol_v = 0 if exact else 2 * ulp32(Q / n) + 2.0 ** -23 * (S / n) ** 2
    m_ref, v_ref = m_ref.float().to(F64), v_ref.float().to(F64)      # the correctly rounded values
    bad = []
    m, v = ops.bn_stats(x)
    rm, rv = torch.zeros(C, device=DEV), torch.zeros(C, device=DEV)
    _, m2, r2 = ops.bn_fwd(x, e["gamma"], e["beta"], None, rm, rv, 1.0, 1e-5, False, True)
    for name, got, ref, tol in (("bn_stats mean", m, m_ref, tol_m), ("bn_stats var", v, v_ref, tol_v),
                                ("bn_fwd mean", m2, m_ref, tol_m), ("bn_fwd running_mean (momentum 1)", rm, m_ref, tol_m),
                                ("bn_fwd running_var (momentum 1)", rv, v_ref * bc.unbiased_factor(rows),
                                 (tol_v + ulp32(v_ref)) * bc.unbiased_factor(rows) + ulp32(v_ref * 2))):
        if not bool(((got.to(F64) - ref).abs() <= tol).all()):
            bad.append("%s (rows %d): worst |diff| %g" % (name, rows, float((got.to(F64) - ref).abs().max())))
    r_ref = (v_ref + 1e-5) ** -0.5
    if not bool(((r2.to(F64) - r_ref).abs() <= 0.5 * r_ref ** 3 * (tol_v + ulp32(v_ref + 1e-5)) + 4 * ulp32(r_ref)).all()):
        bad.append("bn_fwd rstd (rows %d): worst |diff| %g" % (rows, float((r2.to(F64) - r_ref).abs().max())))
    return bad


@pytest.mark.parametrize("dtype", [F32, BF], ids=dn)
@pytest.mark.parametrize("C", [8, 16, 64])
def test_exact_every_row_count_1_to_1300(C, dtype):
    """dense sweep: needs no knowledge of the lane mapping.  One map, every prefix of its rows; the references of
    all prefixes are cumulative sums"""
    from ssl4gie_amd import ops
    R = 1300
    e = exact_inputs(R, C, dtype, 5 * C)
    x, dy, y, mean, rstd = e["x"], e["dy"], e["y"], e["mean"], e["rstd"]
    a = rstd.to(F64) * e["gamma"].to(F64)
    masks = {"y": y > 0, "x": x.to(F64) * a + (e["beta"].to(F64) - mean.to(F64) * a) > 0}
    if dtype == BF:
        masks["bits"] = unpack_bits(e["bits"], R, C)    # a prefix of the rows is a prefix of the bytes
    xhat = (x.to(F64) - mean.to(F64)) * rstd.to(F64)
    ref, gs = {}, {}
    for how, mask in masks.items():
        g = torch.where(mask, dy.to(F64), torch.zeros((), dtype=F64, device=DEV))
        assert 2 * float((g * xhat).abs().sum(0).max()) < 2 ** 24
        ref[how], gs[how] = torch.stack([g.cumsum(0), (g * xhat).cumsum(0)], 1), g      # [R, 2, C]
    got = {how: torch.empty(R, 2, C, device=DEV) for how in masks}
    got_tail = torch.empty(R, 2, C, device=DEV)
    dres_ok = torch.ones((), dtype=torch.bool, device=DEV)
    d = x.to(F64) - x[0].to(F64)
    S, Q = d.cumsum(0), (d * d).cumsum(0)
    st = torch.empty(R, 2, C, device=DEV)
    for rows in range(1, R + 1):
        xs, ds = x[:rows], dy[:rows]
        got["y"][rows - 1], dres = ops.bn_bwd_reduce(ds, y[:rows], xs, mean, rstd, True, True)
        dres_ok &= (dres.to(F64) == gs["y"][:rows]).all()
        got["x"][rows - 1] = ops.bn_bwd_reduce_xmask(ds, xs, e["gamma"], e["beta"], mean, rstd)
        if dtype == BF:
            got["bits"][rows - 1], dres = ops.bn_bwd_reduce_bits(ds, e["bits"][:rows * C // 8], xs, mean, rstd)
            dres_ok &= (dres.to(F64) == gs["bits"][:rows]).all()
        dg, db = e["dg0"].clone(), e["db0"].clone()     # the one-call form's tail, accumulating on odd row counts
        ops.bn_bwd(ds, y[:rows], xs, e["gamma"], mean, rstd, True, False, dg, db, bool(rows & 1))
        got_tail[rows - 1, 0], got_tail[rows - 1, 1] = db, dg
        st[rows - 1, 0], st[rows - 1, 1] = ops.bn_stats(xs)
    for how in masks:
        diff = (got[how].to(F64) != ref[how]).flatten(1).any(1).nonzero().flatten().tolist()
        assert not diff, "mask from %s: sums differ from the integer sums at rows = %s" % (how, [r + 1 for r in diff][:20])
    odd = (torch.arange(1, R + 1, device=DEV) & 1).to(F64).view(R, 1, 1)
    tail_ref = ref["y"] + odd * torch.stack([e["db0"], e["dg0"]]).to(F64)
    diff = (got_tail.to(F64) != tail_ref).flatten(1).any(1).nonzero().flatten().tolist()
    assert not diff, "bn_bwd dbeta / dgamma differ at rows = %s" % [r + 1 for r in diff][:20]
    assert bool(dres_ok), "dres is not the masked gradient"
    n = torch.arange(1, R + 1, device=DEV, dtype=F64).view(R, 1)
    m_ref, v_ref = (x[0].to(F64) + S / n).float(), (Q / n - (S / n) ** 2).float()    # correctly rounded
    bad = ((st[:, 0].to(F64) - m_ref).abs() > 2 * ulp32(torch.maximum((S / n).abs(), m_ref.abs()))).any(1)
    assert not bool(bad.any()), "bn_stats mean beyond 2 ulp at rows = %s" % (bad.nonzero().flatten() + 1).tolist()[:20]
    bad = ((st[:, 1].to(F64) - v_ref).abs() > 2 * ulp32(Q / n) + 2.0 ** -23 * (S / n) ** 2).any(1)   # see exact_statistics
    assert not bool(bad.any()), "bn_stats var beyond 2 ulp at rows = %s" % (bad.nonzero().flatten() + 1).tolist()[:20]
    p2 = [r - 1 for r in (1, 2, 4, 8, 16, 32, 64, 128, 256, 512, 1024)]    # |S| <= 8 n: S^2 < 2^24 up to n = 512
    p2 = [r for r in p2 if float(S[r].abs().max()) ** 2 < 2 ** 24]
    assert len(p2) >= 9, p2
    assert torch.equal(st[p2, 0], m_ref[p2]), "bn_stats mean at power-of-two row counts"
    assert torch.equal(st[p2, 1], v_ref[p2]), "bn_stats var at power-of-two row counts"


@pytest.mark.parametrize("dtype", [F32, BF], ids=dn)
@pytest.mark.parametrize("C", bc.EDGE_C)
def test_exact_lane_folding_and_row_edges(C, dtype):
    bad = []
    for rows in bc.edge_rows(C, dtype):
        bad += ["rows=%d %s" % (rows, b) for b in exact_backward(rows, C, dtype, rows + C)]
        bad += exact_statistics(rows, C, dtype, rows + C + 1)
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("dtype", [F32, BF], ids=dn)
@pytest.mark.parametrize("rows,C,parts", bc.PARTITION_SHAPES,
                         ids=["%dparts-%s" % (p, tail_of(p)) for _, _, p in bc.PARTITION_SHAPES])
def test_exact_direct_path_partitions(rows, C, parts, dtype):
    assert bc.bn_parts(rows, C) == parts
    bad = exact_backward(rows, C, dtype, parts) + exact_statistics(rows, C, dtype, parts + 1)
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("rows,C,affine", bc.PRODUCTION,
                         ids=["%dx%d-%s" % (r, C, tail_of(bc.bn_parts(r, C))) for r, C, _ in bc.PRODUCTION])
def test_exact_production_maps_bf16(rows, C, affine):
    bad = exact_backward(rows, C, BF, rows + C) + exact_statistics(rows, C, BF, rows + C + 1)
    torch.cuda.empty_cache()
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("parts", bc.PARTIAL_COUNTS, ids=["%dpartials-%s" % (p, tail_of(p)) for p in bc.PARTIAL_COUNTS])
def test_exact_statistics_from_integer_partials(parts):
    """partials s in {-1, 0, 1}, q in {0, 1, 2} (wider for few partials): S and Q are integers whatever the order of the
    adds, so mean = fl(S / n) and var = fl(fl(Q / n) - fl(d d)): within 2 ulp of the larger term for n = 128 parts - 3;
    equal to the correctly rounded fp64 value for a power-of-two n (S / n, Q / n and d d exact: S^2 < 2^24)"""
    from ssl4gie_amd import ops
    C = 200 if parts <= 2049 else 64
    g = torch.Generator(DEV).manual_seed(parts)
    w = 16 if parts <= 64 else 1
    p = torch.stack([ints(g, (parts, C), -w, w, F32), ints(g, (parts, C), w * w, 2 * w * w, F32)], 1).contiguous()
    S, Q = p[:, 0].to(F64).sum(0), p[:, 1].to(F64).sum(0)
    assert float(p.abs().to(F64).sum(0).max()) < 2 ** 24 and float(S.abs().max()) ** 2 < 2 ** 24
    gamma, beta = pick(g, [-2.0, 0.0, 1.0, 3.0], C), pick(g, [-1.0, 0.0, 1.0], C)
    n2 = 1 << max(7, (parts * w * w * 2 - 1).bit_length())      # Q / n <= 1 ... and var >= 0 for either n
    bad = []
    for rows in (max(parts * 128 - 3, 1), n2):
        n = float(rows)
        m_ref, v_ref = S / n, (Q / n - (S / n) ** 2).clamp_min(0)
        if rows == n2:
            tol_m = tol_v = torch.zeros_like(m_ref)
        else:
            tol_m, tol_v = 2 * ulp32(m_ref), 2 * ulp32(Q / n)
        m_ref, v_ref = m_ref.float().to(F64), v_ref.float().to(F64)      # the correctly rounded values
        r_ref = (v_ref + 1e-5) ** -0.5
        tol_r = 0.5 * r_ref ** 3 * (tol_v + ulp32(v_ref + 1e-5)) + 4 * ulp32(r_ref)
        x = torch.zeros(rows, C, dtype=BF, device=DEV)
        outs = {}
        outs["bn_stats(partials)"] = ops.bn_stats(x, partials=p) + (None,)
        rm, rv = torch.zeros(C, device=DEV), torch.zeros(C, device=DEV)
        _, m, r = ops.bn_fwd(x, gamma, beta, None, rm, rv, 1.0, 1e-5, False, True, partials=p)
        outs["bn_fwd(partials)"] = (m, None, r)
        outs["bn_fwd(partials) running (momentum 1)"] = (rm, None, None)
        _, _, m, r = ops.bn_fwd_bits(x, gamma, beta, None, None, None, 0.1, 1e-5, p)
        outs["bn_fwd_bits"] = (m, None, r)
        coef, m, r = ops.bn_coef_partials(p, rows, gamma, beta, None, None, 0.1, 1e-5)
        outs["bn_coef_partials"] = (m, None, r)
        a_ref = r.to(F64) * gamma.to(F64)
        if not bool(((coef[0].to(F64) - a_ref).abs() <= ulp32(a_ref)).all() and
                    ((coef[1].to(F64) - (beta.to(F64) - m.to(F64) * a_ref)).abs()
                     <= 2 * ulp32(beta.to(F64).abs() + (m.to(F64) * a_ref).abs())).all()):
            bad.append("bn_coef_partials coef (rows %d)" % rows)
        for name, (m, v, r) in outs.items():
            for what, got, ref, tol in (("mean", m, m_ref, tol_m), ("var", v, v_ref, tol_v), ("rstd", r, r_ref, tol_r)):
                if got is not None and not bool(((got.to(F64) - ref).abs() <= tol).all()):
                    err = (got.to(F64) - ref).abs()
                    bad.append("%s %s (rows %d): worst |diff| %g at channel %d" % (name, what, rows, float(err.max()), int(err.argmax())))
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("rows,C", [(1, 8), (5, 24), (77, 520), (4099, 64), (12544, 2048)])
def test_exact_apply_bits(rows, C):
    """coefficients and operands chosen so that y is exact in bf16: y equals the fp64 value and the bit map is
    y > 0 of the stored y (zeros, negative zeros and clamped negatives are 0 bits)"""
    from ssl4gie_amd import ops
    g = torch.Generator(DEV).manual_seed(rows + C)
    x, res = ints(g, (rows, C), -4, 4, BF), ints(g, (rows, C), -3, 3, BF)
    coef = torch.stack([pick(g, [-2.0, -1.0, -0.5, 0.0, 0.5, 1.0, 2.0], C), pick(g, [-2.0, -1.0, 0.0, 0.5, 1.0], C)]).contiguous()
    for r in (None, res):
        y, bits = ops.bn_apply_bits(x, coef, r)
        ref = x.to(F64) * coef[0].to(F64) + coef[1].to(F64) + (0 if r is None else r.to(F64))
        assert torch.equal(y.to(F64), ref.clamp_min(0))
        assert torch.equal(bits, pack_bits(y > 0)) and torch.equal(unpack_bits(bits, rows, C), ref > 0)


@pytest.mark.parametrize("C", [8, 200, 2048])
@pytest.mark.parametrize("world", [1, 2, 8])
def test_combine_stats_unequal_ranks(world, C):
    """ssl4gie_bn_combine_stats against the fp64 pooled mean / variance of ranks with unequal row counts"""
    from ssl4gie_amd import _lib, ops
    g = torch.Generator(DEV).manual_seed(world * C)
    rn = lambda *s: torch.randn(*s, generator=g, device=DEV)
    mean_w, var_w = rn(world, C) + 3 * rn(C), torch.rand(world, C, generator=g, device=DEV) + 0.01
    var_w[:, 3] = 0
    mean_w[:, 3] = 1.5
    rows_w = torch.randint(1, 5000, (world, 1), generator=g, device=DEV).float()
    gathered = torch.cat([mean_w, var_w, rows_w], 1).contiguous()
    rm0, rv0 = rn(C), torch.rand(C, generator=g, device=DEV) + 0.5
    rm, rv = rm0.clone(), rv0.clone()
    out = torch.empty(2 * C + 1, device=DEV)
    _lib.check(_lib.load().ssl4gie_bn_combine_stats(gathered.data_ptr(), world, C, 1e-5, 0.1, rm.data_ptr(), rv.data_ptr(),
                                                    out[:C].data_ptr(), out[C:2 * C].data_ptr(), out[2 * C:].data_ptr(),
                                                    ops.stream()), "bn_combine_stats")
    total = rows_w.to(F64).sum()
    assert float(out[2 * C]) == float(total)
    wgt = rows_w.to(F64) / total
    mean = (mean_w.to(F64) * wgt).sum(0)
    var = ((var_w.to(F64) + (mean_w.to(F64) - mean) ** 2) * wgt).sum(0)
    t_mean = (mean_w.to(F64).abs() * wgt).sum(0)
    st = {"mean": mean, "var": var, "t_mean": t_mean, "n": float(total),
          "t_var": ((var_w.to(F64) + (mean_w.to(F64).abs() + mean.abs() + t_mean) ** 2) * wgt).sum(0)}
    rep = bc.Report()
    bc.check_stats(rep, st, 1e-5, out[:C], None, out[C:2 * C], (rm, rv, rm0, rv0, 0.1))
    finish(rep)
