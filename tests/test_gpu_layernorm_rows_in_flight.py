"""Rows in flight in the LayerNorm kernels of norm.hip: the forward is a persistent grid whose waves walk rows
w, w + W, ... with the next row's loads issued before the current row is reduced; the backward's waves do the same
over their grid-stride loop (whole rows up to 512 columns, the residual gradient with dy and x beyond).  None of
that may be visible in a result:

  row independence   a row of one launch over R rows equals, bit for bit, the launch over that row alone — the first
                     and the last row, rows of a wave's second and last loop trip, the rows before and after a
                     multiple of W (a look-ahead past `rows`, a skipped or doubled row at the loop's tail, the two
                     register sets exchanged);
  guard bands        inputs followed by NaN, outputs by a sentinel: outputs finite, sentinels untouched (a look-ahead
                     of a row that does not exist is not issued at all);
  partial rows       dgamma / dbeta bit-equal between two runs, and within ln_checks' bound of the fp64 reference.

W, the waves of a launch, is derived as the launch derives it: forward 4 waves x min(ceil(R / 4), resident workgroups
per CU of the instantiation x the library's compute CUs (240, ssl4gie_set_compute_cus)); backward 4 x min(ceil(R / 4),
1024).  Through the C ABI, as ops.layernorm_fwd / layernorm_bwd call it, on buffers the test owns (the guard bands
and the dx-only call need them)."""
import pytest
import torch

import ln_checks as lc

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32, BF = torch.float32, torch.bfloat16
COMPUTE_CUS = 240
FWD_PER_CU = {1: 8, 2: 6, 3: 5, 4: 4, 8: 2}     # norm.hip: ln_fwd_per_cu
SENTINEL = -12288.0  # exact in bf16
GUARD = 4096        # elements of slack after the last row: pages of it at every width


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from ssl4gie_amd import _lib
    assert _lib.load().ssl4gie_set_compute_cus(COMPUTE_CUS) == 0


def fwd_waves(cols):
    nv = (cols + 255) // 256
    return 4 * FWD_PER_CU[nv if nv <= 4 else 8] * COMPUTE_CUS


BWD_WAVES = 4 * 1024


def row_counts(W):
    return sorted({1, 3, 4, 5, W - 1, W, W + 1, 3 * W + 2})


def selected_rows(R, W):
    """first, last, a row of the second and of the last trip of a wave, the rows around every multiple of W"""
    last_trip = (R - 1) // W * W
    rows = {0, R - 1, W + 1, last_trip, last_trip + (R - 1 - last_trip) // 2}
    for k in range(1, R // W + 1):
        rows |= {k * W - 1, k * W}
    return sorted(r for r in rows if 0 <= r < R)


def guarded(rows, cols, dtype, fill):
    """a [rows, cols] view at the head of a buffer whose remaining GUARD elements hold `fill`"""
    buf = torch.full((rows * cols + GUARD,), fill, dtype=dtype, device=DEV)
    return buf, buf[:rows * cols].view(rows, cols)


def make_inputs(R, cols, dt, seed):
    g = torch.Generator(DEV).manual_seed(seed)
    nan = float("nan")
    t = {}
    for name, dtype in (("x", F32), ("dy", dt), ("dres", F32)):
        t[name + "_buf"], v = guarded(R, cols, dtype, nan)
        v.copy_(torch.randn(R, cols, generator=g, device=DEV) * (1.5 if name == "x" else 1.0) + (0.5 if name == "x" else 0.0))
        t[name] = v
    t["gamma"] = torch.randn(cols, generator=g, device=DEV)
    t["beta"] = 0.3 * torch.randn(cols, generator=g, device=DEV)
    return t


def fwd_raw(x, gamma, beta, y, mean, rstd, rows, cols):
    from ssl4gie_amd import _lib, ops
    rc = _lib.load().ssl4gie_layernorm_fwd(ops.ptr(x), ops.ptr(gamma), ops.ptr(beta), ops.ptr(y), ops.code(y.dtype),
                                           ops.ptr(mean), ops.ptr(rstd), rows, cols, 1e-6, ops.stream())
    assert rc == 0


def bwd_raw(dy, x, gamma, mean, rstd, dres, dx, dx_lp, rows, cols, dgamma=None, dbeta=None):
    from ssl4gie_amd import _lib, ops
    L = _lib.load()
    ws = torch.empty(max(16, L.ssl4gie_layernorm_bwd_workspace_bytes(rows, cols)), dtype=torch.uint8, device=DEV)
    rc = L.ssl4gie_layernorm_bwd(ops.ptr(dy), ops.code(dy.dtype), ops.ptr(x), ops.ptr(gamma), ops.ptr(mean),
                                 ops.ptr(rstd), ops.ptr(dres), ops.ptr(dx), ops.ptr(dx_lp), ops.code(dy.dtype),
                                 ops.ptr(dgamma), ops.ptr(dbeta), 0, ops.ptr(ws), rows, cols, ops.stream())
    assert rc == 0


def run_fwd(t, R, cols, dt):
    o = {}
    o["y_buf"], o["y"] = guarded(R, cols, dt, SENTINEL)
    o["mean_buf"], o["rstd_buf"] = (torch.full((R + GUARD,), SENTINEL, device=DEV) for _ in range(2))
    o["mean"], o["rstd"] = o["mean_buf"][:R], o["rstd_buf"][:R]
    fwd_raw(t["x"], t["gamma"], t["beta"], o["y"], o["mean"], o["rstd"], R, cols)
    return o


def run_bwd(t, o, R, cols, dt, sums=False):
    o["dx_buf"], o["dx"] = guarded(R, cols, F32, SENTINEL)
    o["dx_lp_buf"], o["dx_lp"] = guarded(R, cols, dt, SENTINEL)
    if sums:
        o["dgamma"], o["dbeta"] = (torch.full((cols,), float("nan"), device=DEV) for _ in range(2))
    bwd_raw(t["dy"], t["x"], t["gamma"], o["mean"], o["rstd"], t["dres"], o["dx"], o["dx_lp"], R, cols,
            o.get("dgamma"), o.get("dbeta"))
    return o


def same(name, got, want, where):
    assert got.dtype == want.dtype and torch.equal(got, want), \
        "%s of %s differs from the launch over that row alone" % (name, where)


def check_guards(o, R, cols, names, where):
    for n in names:
        body = o[n]
        assert bool(torch.isfinite(body.float()).all()), "%s of %s is not finite" % (n, where)
        tail = o[n + "_buf"][body.numel():]
        assert tail.numel() == GUARD and bool((tail.float() == SENTINEL).all()), \
            "%s of %s: written past the last row" % (n, where)


FWD_BWD_COLS = (4, 252, 512, 768, 1020, 1024)


@pytest.mark.parametrize("dt", [BF, F32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("cols", FWD_BWD_COLS + (2048,))
def test_forward_rows_independent(cols, dt):
    W = fwd_waves(cols)
    for R in row_counts(W):
        where = "forward %dx%d (W = %d)" % (R, cols, W)
        t = make_inputs(R, cols, dt, seed=cols + R)
        o = run_fwd(t, R, cols, dt)
        if R in (1, W + 1):
            check_guards(o, R, cols, ("y", "mean", "rstd"), where)
        for r in selected_rows(R, W):
            y1 = torch.empty(1, cols, dtype=dt, device=DEV)
            m1, r1 = torch.empty(1, device=DEV), torch.empty(1, device=DEV)
            fwd_raw(t["x"][r:r + 1], t["gamma"], t["beta"], y1, m1, r1, 1, cols)
            same("y", o["y"][r:r + 1], y1, where + " row %d" % r)
            same("mean", o["mean"][r:r + 1], m1, where + " row %d" % r)
            same("rstd", o["rstd"][r:r + 1], r1, where + " row %d" % r)
        del t, o


@pytest.mark.parametrize("dt", [BF, F32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("cols", FWD_BWD_COLS)
def test_backward_rows_independent(cols, dt):
    """the dx-only call (dgamma = dbeta = NULL), with dres and dx_lp"""
    W = BWD_WAVES
    for R in row_counts(W):
        where = "backward %dx%d (W = %d)" % (R, cols, W)
        t = make_inputs(R, cols, dt, seed=7 * cols + R)
        o = run_bwd(t, run_fwd(t, R, cols, dt), R, cols, dt)
        if R in (1, W + 1):
            check_guards(o, R, cols, ("dx", "dx_lp"), where)
        for r in selected_rows(R, W):
            s = slice(r, r + 1)
            dx1 = torch.empty(1, cols, device=DEV)
            lp1 = torch.empty(1, cols, dtype=dt, device=DEV)
            bwd_raw(t["dy"][s], t["x"][s], t["gamma"], o["mean"][s], o["rstd"][s], t["dres"][s], dx1, lp1, 1, cols)
            same("dx", o["dx"][s], dx1, where + " row %d" % r)
            same("dx_lp", o["dx_lp"][s], lp1, where + " row %d" % r)
        del t, o


@pytest.mark.parametrize("dt", [BF, F32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("cols", FWD_BWD_COLS)
def test_partial_rows_repeatable_and_within_bound(cols, dt):
    """dgamma / dbeta of two runs over the same inputs, bit for bit, and against fp64 within ln_checks' k: a case of
    ln_checks (generated on the CPU) at 3 W + 2 rows for the production widths and W + 1 for the others"""
    R = (3 if cols in (512, 768) else 1) * BWD_WAVES + (2 if cols in (512, 768) else 1)
    c = lc.to_device(lc.row_case("gauss", R, cols, dt, dt, True, False), DEV)
    t = {"x": c["x"], "dy": c["dy"], "dres": c["dres"], "gamma": c["gamma"], "beta": c["beta"]}
    o = run_bwd(t, run_fwd(t, R, cols, dt), R, cols, dt, sums=True)
    o2 = run_bwd(t, dict(o), R, cols, dt, sums=True)
    for n in ("dgamma", "dbeta", "dx", "dx_lp"):
        assert torch.equal(o[n], o2[n]), "%s differs between two runs of %dx%d" % (n, R, cols)
    rep = lc.Report(tag="rows in flight %dx%d" % (R, cols))
    lc.check_row_backward(rep, c["dy"], c["x"], c["gamma"], o["mean"], o["rstd"], c["dres"], o["dx"], o["dx_lp"],
                          o["dgamma"], o["dbeta"])
    print("\n%dx%d %s worst error / (2^-24 mag):" % (R, cols, dt), {n: float("%.3g" % v) for n, v in sorted(rep.worst.items())})
    rep.assert_ok()
