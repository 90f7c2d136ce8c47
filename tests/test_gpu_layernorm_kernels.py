"""The LayerNorm kernels of norm.hip (row forward / backward, reduce_partials_kernel, the three column-sum kernels),
the map LayerNorm of det_ops.hip and the two small reductions that share reduce_partials_kernel, against a plain
fp64 reference, per element (tests/ln_checks.py: the reference, the bounds, how their constants were derived and
the case list; tests/test_ln_checks_cpu.py: proof that the checks bite).  Through ssl4gie_amd.ops, and through the
C ABI directly where the wrapper hides an argument (ld of ssl4gie_colsum, NULL dgamma / dbeta, rows = 0).

Case list (ln_checks.gpu_*_specs): every column count on both sides of a vector strip, 37 rows, six input families,
fp32 / bf16 y, dy and dx_lp, dres and dx_lp given or NULL, overwrite and accumulate; rows on every boundary of the
launch geometry (a partial block, the grid-stride loop from 4097 rows, nparts = 15 .. 1024 of the partial-row
reduction); the production shapes, with the fp64 reference on the device; the block executor with and without the
weight-gradient side stream; map sizes from 8 elements to three strides of the reduce loop and the pyramid's own
maps, with an outlier at and next to element 0; column sums with ld > cols, an unaligned base and rows = 0.

Run time on an MI355X: not yet measured (the module has not run on a device)."""
import os

import pytest
import torch

import ln_checks as lc

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32, BF, F64 = torch.float32, torch.bfloat16, torch.float64
EARG = 1000
WORST = {}      # worst error / (2^-24 mag) per check over the module (printed by the last test)


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from ssl4gie_amd import _lib
    _lib.load()


def done(rep):
    for n, v in rep.worst.items():
        WORST[n] = max(WORST.get(n, 0.0), v)
    rep.assert_ok()


def of_group(specs, group):
    return [s for s in specs if s[0] == group]


ROW_SPECS, FWD_SPECS = list(lc.gpu_row_specs()), list(lc.gpu_fwd_only_specs())
MAP_SPECS, COLSUM_SPECS = list(lc.gpu_map_specs()), list(lc.gpu_colsum_specs())


# ===================================================================== row LayerNorm
def ln_bwd_raw(c, mean, rstd, dx, dx_lp=None, lp_dtype=None, dgamma=None, dbeta=None, accumulate=0, rows=None, cols=None):
    from ssl4gie_amd import _lib, ops
    L = _lib.load()
    rows, cols = c["rows"] if rows is None else rows, c["cols"] if cols is None else cols
    ws = torch.empty(max(16, L.ssl4gie_layernorm_bwd_workspace_bytes(max(rows, 1), c["cols"])), dtype=torch.uint8, device=DEV)
    dyc = ops.code(c["dy"].dtype)
    rc = L.ssl4gie_layernorm_bwd(ops.ptr(c["dy"]), dyc, ops.ptr(c["x"]), ops.ptr(c["gamma"]), ops.ptr(mean), ops.ptr(rstd),
                                 ops.ptr(c["dres"]), ops.ptr(dx), ops.ptr(dx_lp), dyc if lp_dtype is None else ops.code(lp_dtype),
                                 ops.ptr(dgamma), ops.ptr(dbeta), accumulate, ops.ptr(ws), rows, cols, ops.stream())
    torch.cuda.synchronize()
    return rc


def run_row(spec, rep, null_sums=False):
    from ssl4gie_amd import ops
    _, a, lp = spec
    c = lc.to_device(lc.row_case(*a), DEV)
    tag = "%s %dx%d y:%s dy:%s dres:%d lp:%d acc:%d" % (a[0], a[1], a[2], a[3], a[4], a[5], lp, a[6])
    y, mean, rstd = ops.layernorm_fwd(c["x"], c["gamma"], c["beta"], c["eps"], c["y_dtype"])
    y2, m2, r2 = ops.layernorm_fwd(c["x"], c["gamma"], c["beta"], c["eps"], c["y_dtype"], save_stats=False)
    assert m2 is None and r2 is None
    acc = c["dg0"] is not None
    dg = c["dg0"].clone() if acc else None
    db = c["db0"].clone() if acc else None
    dx, dx_lp, dg, db = ops.layernorm_bwd(c["dy"], c["x"], c["gamma"], mean, rstd, dres=c["dres"], want_lp=lp,
                                          dgamma=dg, dbeta=db, accumulate=acc)
    assert (dx_lp is not None) == lp and (dx_lp is None or dx_lp.dtype == c["dy_dtype"])
    r = lc.check_row_all(c, {"y": y, "mean": mean, "rstd": rstd, "dx": dx, "dx_lp": dx_lp, "dgamma": dg, "dbeta": db},
                         tag=tag)
    r.same("y_nostats", y2, y, "y without saved statistics differs")
    if null_sums:       # dgamma == dbeta == NULL (the block executor's call): the same dx, nothing else written
        dx3 = torch.full_like(dx, float("nan"))
        assert ln_bwd_raw(c, mean, rstd, dx3) == 0
        r.same("dx_null_sums", dx3, dx, "dx differs without dgamma / dbeta")
    rep.merge(r)


@pytest.mark.parametrize("group", lc.groups(s for s in ROW_SPECS if s[0].startswith("cols")))
def test_row_fwd_bwd_every_column_count(group):
    rep = lc.Report()
    for spec in of_group(ROW_SPECS, group):
        run_row(spec, rep)
    done(rep)


@pytest.mark.parametrize("group", lc.groups(FWD_SPECS))
def test_row_fwd_wide_columns(group):
    """1025 .. 2048 columns: the forward's eight-strip instantiation (the backward stops at 1024)"""
    from ssl4gie_amd import ops
    rep = lc.Report()
    for _, a in of_group(FWD_SPECS, group):
        c = lc.to_device(lc.row_case(*a), DEV)
        y, mean, rstd = ops.layernorm_fwd(c["x"], c["gamma"], c["beta"], c["eps"], c["y_dtype"])
        y2, _, _ = ops.layernorm_fwd(c["x"], c["gamma"], c["beta"], c["eps"], c["y_dtype"], save_stats=False)
        r = lc.Report(tag="%s %dx%d y:%s" % (a[0], a[1], a[2], a[3]))
        lc.check_row_forward(r, c["x"], c["gamma"], c["beta"], c["eps"], y, mean, rstd)
        r.same("y_nostats", y2, y, "y without saved statistics differs")
        rep.merge(r)
    done(rep)


@pytest.mark.parametrize("group", lc.groups(s for s in ROW_SPECS if s[0].startswith("geometry")))
def test_row_launch_geometry(group):
    rep = lc.Report()
    for spec in of_group(ROW_SPECS, group):
        run_row(spec, rep, null_sums=True)
    done(rep)


@pytest.mark.parametrize("group", lc.groups(s for s in ROW_SPECS if s[0].startswith("production")))
def test_row_production_shapes(group):
    rep = lc.Report()
    for spec in of_group(ROW_SPECS, group):
        run_row(spec, rep)
        torch.cuda.empty_cache()
    done(rep)


def test_row_rejections_and_zero_rows():
    """what the interface refuses it refuses before any launch (SSL4GIE_EARG, nothing written); rows = 0 succeeds
    and writes nothing.  Every buffer is large enough for the call as it would run if it were accepted."""
    from ssl4gie_amd import _lib, ops
    L = _lib.load()
    rows = 8
    big = lambda dtype=F32: torch.full((rows, 2056), 7.0, dtype=dtype, device=DEV)
    x, y, ybf, dy, dybf, dres, dx, dxlp, dxlpbf = big(), big(), big(BF), big(), big(BF), big(), big(), big(), big(BF)
    gamma, beta, dg, db = (torch.full((2056,), 7.0, device=DEV) for _ in range(4))
    mean, rstd = torch.full((rows,), 7.0, device=DEV), torch.full((rows,), 7.0, device=DEV)
    ws = torch.empty(L.ssl4gie_layernorm_bwd_workspace_bytes(rows, 2056), dtype=torch.uint8, device=DEV)
    outs = (y, ybf, dx, dxlp, dxlpbf, dg, db, mean, rstd)

    def fwd(r, cols, yt=F32):
        return L.ssl4gie_layernorm_fwd(ops.ptr(x), ops.ptr(gamma), ops.ptr(beta), ops.ptr(y if yt == F32 else ybf),
                                       ops.code(yt), ops.ptr(mean), ops.ptr(rstd), r, cols, 1e-6, ops.stream())

    def bwd(r, cols, dyt=F32, lpt=F32, lp=True):
        return L.ssl4gie_layernorm_bwd(ops.ptr(dy if dyt == F32 else dybf), ops.code(dyt), ops.ptr(x), ops.ptr(gamma),
                                       ops.ptr(mean), ops.ptr(rstd), ops.ptr(dres), ops.ptr(dx),
                                       ops.ptr((dxlp if lpt == F32 else dxlpbf) if lp else None), ops.code(lpt),
                                       ops.ptr(dg), ops.ptr(db), 0, ops.ptr(ws), r, cols, ops.stream())
    assert fwd(0, 768) == 0 and fwd(0, 768, BF) == 0 and bwd(0, 768) == 0 and bwd(0, 768, BF, BF) == 0
    for cols in (6, 1026, 2052, 2056):
        assert fwd(rows, cols) == EARG, cols
        assert fwd(rows, cols, BF) == EARG, cols
    for cols in (6, 1026, 1028, 2048):
        assert bwd(rows, cols) == EARG, cols
        assert bwd(rows, cols, BF, BF) == EARG, cols
    assert bwd(rows, 768, BF, F32) == EARG and bwd(rows, 768, F32, BF) == EARG
    torch.cuda.synchronize()
    for t in outs:
        assert bool((t == 7.0).all())
    assert bwd(rows, 768, F32, BF, lp=False) == 0      # without dx_lp its type is not looked at
    torch.cuda.synchronize()


# ===================================================================== block executor
@pytest.mark.parametrize("dt,D,H", [(BF, 384, 6), (F32, 192, 3)], ids=["bf16-384", "fp32-192"])
def test_block_stack_ln_gradients_same_with_and_without_side_stream(dt, D, H):
    """the weight-gradient side stream hands LayerNorm's partial rows to a second-stage reduction on another stream,
    over two workspaces reused block after block; folded back onto the caller's stream it launches the same kernels
    on the same partial rows: the LayerNorm parameter gradients and x.grad must agree bit for bit (T = 4728 rows:
    the grid-stride loop and 1024 partial rows)"""
    import torch.nn as nn
    from ssl4gie_amd import _lib, engine
    from ssl4gie_amd.Models.vit_layers import Block
    L = _lib.load()
    B, N, depth = 24, 197, 3
    torch.manual_seed(11)
    blocks = nn.ModuleList([Block(D, H, 4.0, qkv_bias=True, norm_layer=lambda d: nn.LayerNorm(d, eps=1e-6))
                            for _ in range(depth)]).to(DEV)
    g = torch.Generator("cpu").manual_seed(12)
    x = torch.randn(B, N, D, generator=g).to(DEV)
    wgt = torch.randn(B, N, D, generator=g).to(DEV)
    ln_names = [n for n, _ in blocks.named_parameters() if ".norm1." in n or ".norm2." in n]
    assert len(ln_names) == 4 * depth
    as_loaded = 0 if os.environ.get("SSL4GIE_WGRAD_STREAM", "")[:1] == "0" else 1
    res = []
    try:
        for setting in (None, 0):
            if setting is not None:
                assert L.ssl4gie_set_wgrad_stream(setting) == 0
            for p in blocks.parameters():
                p.grad = None
            xi = x.clone().requires_grad_(True)
            y, _ = engine.run_blocks(blocks, xi, H, 1e-6, dt, engine.GradSink(None))
            (y * wgt).sum().backward()
            torch.cuda.synchronize()
            grads = dict((n, p.grad.clone()) for n, p in blocks.named_parameters())
            res.append((y.detach().clone(), xi.grad.clone(), grads))
    finally:
        L.ssl4gie_set_wgrad_stream(as_loaded)
    assert torch.equal(res[0][0], res[1][0])
    assert torch.equal(res[0][1], res[1][1]), "x.grad differs"
    for n in ln_names:
        a, b = res[0][2][n], res[1][2][n]
        assert bool(torch.isfinite(a).all()) and float(a.abs().max()) > 0, n
        assert torch.equal(a, b), (n, float((a - b).abs().max()))


# ===================================================================== map LayerNorm
@pytest.mark.parametrize("group", lc.groups(MAP_SPECS))
def test_map_layernorm(group):
    from ssl4gie_amd import ops
    rep = lc.Report()
    for _, a in of_group(MAP_SPECS, group):
        c = lc.to_device(lc.map_case(*a), DEV)
        y, mean, rstd = ops.map_layernorm_fwd(c["x"], c["w"], c["bias"], c["eps"])
        acc = c["dw0"] is not None
        dw = c["dw0"].clone() if acc else torch.full_like(c["w"], float("nan"))
        db = c["db0"].clone() if acc else torch.full_like(c["w"], float("nan"))
        dx = ops.map_layernorm_bwd(c["x"], c["dy"], c["w"], mean, rstd, dw, db, accumulate=acc)
        r = lc.check_map_all(c, {"y": y, "mean": mean, "rstd": rstd, "dx": dx, "dw": dw, "db": db},
                             tag="map %s %s B%d acc:%d" % (a[0], group, a[1], acc))
        dx2 = ops.map_layernorm_bwd(c["x"], c["dy"], c["w"], mean, rstd, None, None)       # dw == db == NULL
        r.same("map_dx_null_sums", dx2, dx, "dx differs without dw / db")
        dw2 = torch.full_like(c["w"], float("nan"))
        ops.map_layernorm_bwd(c["x"], c["dy"], c["w"], mean, rstd, dw2, None)              # db alone NULL
        if not acc:
            r.same("map_dw_alone", dw2, dw, "dw differs without db")
        rep.merge(r)
        del c, y, dx, dx2, dw, db, dw2
    torch.cuda.empty_cache()
    done(rep)


# ===================================================================== column sums
def colsum_raw(base_ptr, dtype, out, accumulate, rows, cols, ld):
    from ssl4gie_amd import _lib, ops
    L = _lib.load()
    ws = torch.empty(max(16, L.ssl4gie_colsum_workspace_bytes(rows, cols)), dtype=torch.uint8, device=DEV)
    rc = L.ssl4gie_colsum(base_ptr, ops.code(dtype), ops.ptr(out), int(accumulate), ops.ptr(ws), rows, cols, ld, ops.stream())
    torch.cuda.synchronize()
    return rc


@pytest.mark.parametrize("group", lc.groups(COLSUM_SPECS))
def test_colsum(group):
    """the vector, narrow and scalar kernels, fp32 and bf16; ld = cols overwritten, a window of a wider matrix
    (ld = cols + 24) accumulated; the same window from an unaligned base (one element in: the scalar kernel)"""
    rep = lc.Report()
    for _, a in of_group(COLSUM_SPECS, group):
        c = lc.to_device(lc.colsum_case(*a), DEV)
        rows, cols, ld, wide = c["rows"], c["cols"], c["ld"], c["wide"]
        acc = c["init"] is not None
        out = c["init"].clone() if acc else torch.full((cols,), float("nan"), device=DEV)
        assert colsum_raw(wide.data_ptr(), c["dtype"], out, acc, rows, cols, ld) == 0
        rep.merge(lc.check_colsum_all(c, out, tag="colsum %s %s ld %d %s" % (a[0], group, ld, a[4])))
        if ld > cols:       # columns 1 .. cols of the wide matrix: a base that is not 16-byte aligned
            assert (wide.data_ptr() + wide.element_size()) % 16 != 0
            c2 = dict(c, x=wide[:, 1:1 + cols])
            out = c["init"].clone()
            assert colsum_raw(wide.data_ptr() + wide.element_size(), c["dtype"], out, True, rows, cols, ld) == 0
            rep.merge(lc.check_colsum_all(c2, out, tag="colsum unaligned %s ld %d %s" % (group, ld, a[4])))
    done(rep)


@pytest.mark.parametrize("cols", [4, 64, 130, 384, 6])
@pytest.mark.parametrize("dtype", [F32, BF], ids=["fp32", "bf16"])
def test_colsum_zero_rows(cols, dtype):
    x = torch.ones(4, cols, dtype=dtype, device=DEV)        # a valid pointer: nothing of it is to be read
    out = torch.full((cols,), float("nan"), device=DEV)
    assert colsum_raw(x.data_ptr(), dtype, out, False, 0, cols, cols) == 0
    assert torch.equal(out, torch.zeros(cols, device=DEV))
    init = torch.randn(cols, generator=torch.Generator("cpu").manual_seed(cols)).to(DEV)
    out = init.clone()
    assert colsum_raw(x.data_ptr(), dtype, out, True, 0, cols, cols) == 0
    assert torch.equal(out, init)


# ===================================================================== the small reductions of the MAE step
@pytest.mark.parametrize("accumulate", [False, True], ids=["overwrite", "accumulate"])
def test_assemble_backward_reductions_production_shape(accumulate):
    """dcls = sum_b dx[b, 0] (tokens_assemble_bwd) and dmask_token = the sum of the removed rows
    (decoder_assemble_bwd: B * 8 partial rows through reduce_partials_kernel) at B = 256, L = 196, nkeep = 49, D = 512"""
    from ssl4gie_amd import ops
    B, Lp, keep, D = 256, 196, 49, 512
    g = torch.Generator("cpu").manual_seed(21)
    rep = lc.Report(tag="assemble_bwd acc:%d" % accumulate)
    dx = torch.randn(B, keep + 1, D, generator=g).to(DEV)
    init = torch.randn(D, generator=g).to(DEV)
    dcls = init.clone() if accumulate else torch.full((D,), float("nan"), device=DEV)
    dy = ops.tokens_assemble_bwd(dx, BF, dcls_out=dcls, accumulate=accumulate)
    lc.check_colsum(rep, dx[:, 0], dcls, init if accumulate else None, name="dcls")
    rep.same("tokens_dy", dy, dx[:, 1:].reshape(-1, D).to(BF), "not the token rows rounded to bf16")
    s, _, _ = ops.mask_argsort(torch.rand(B, Lp, generator=g).to(DEV), keep)
    dxd = torch.randn(B, Lp + 1, D, generator=g).to(DEV)
    dmt = init.clone() if accumulate else torch.full((D,), float("nan"), device=DEV)
    dyd = ops.decoder_assemble_bwd(dxd, s, keep, BF, dmask_out=dmt, accumulate=accumulate)
    pick = lambda ids: dxd[:, 1:].gather(1, ids[:, :, None].expand(-1, -1, D))
    lc.check_colsum(rep, pick(s[:, keep:]).reshape(-1, D), dmt, init if accumulate else None, name="dmask_token")
    rep.same("decoder_dy", dyd, torch.cat([dxd[:, :1], pick(s[:, :keep])], 1).to(BF), "not the kept rows rounded to bf16")
    done(rep)


def test_zz_worst_ratios():
    """not a check: the kernels' worst error / (2^-24 mag) per check over this module, for ln_checks' table"""
    print("\nworst error / (2^-24 mag):", {n: float("%.3g" % v) for n, v in sorted(WORST.items())})
