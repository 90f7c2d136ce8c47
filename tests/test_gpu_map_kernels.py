"""The map and layout kernels of dpt_ops.hip, resnet_ops.hip and det_ops.hip — bilinear x2, the 3x3 / 2x2 max pools,
the average pool, im2col3x3 / col2im3x3, the stem patch matrix, subsample2, pixel (un)shuffle, tokens <-> map, the
pointwise maps, the depth head and the momentum update — against a plain fp64 reference, per element
(tests/map_checks.py: the references, the bounds, how their constants were derived and the case list;
tests/test_map_checks_cpu.py: proof that the checks bite).

Every kernel is called through the C ABI with its outputs in the middle of a buffer that carries 256 sentinel
elements on either side (`Guard`); both bands must be untouched after every case.  Both dtypes wherever they are
accepted; the shapes are the smallest at which each kernel can still go wrong (map_checks.gpu_specs).

Run time on an MI355X: 146 tests in 4 s, none above 0.2 s after the first (which loads the library)."""
import math

import pytest
import torch

import map_checks as mc

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32, BF, F64 = torch.float32, torch.bfloat16, torch.float64
EARG = 1000
SENTINEL, SENTINEL_BYTE, BAND = 12288.0, 0xAB, 256
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


class Guard:
    """outputs with BAND sentinel elements before and after"""

    def __init__(self):
        self.items = []

    def out(self, shape, dtype, init=None):
        n = math.prod(shape)
        fill = SENTINEL_BYTE if dtype == torch.uint8 else SENTINEL
        buf = torch.full((n + 2 * BAND,), fill, dtype=dtype, device=DEV)
        self.items.append((buf, n, fill))
        v = buf[BAND:BAND + n].view(shape)
        if init is not None:
            v.copy_(init)
        return v

    def check(self, tag):
        torch.cuda.synchronize()
        for buf, n, fill in self.items:
            assert bool((buf[:BAND] == fill).all()), "%s: written before the output" % tag
            assert bool((buf[BAND + n:] == fill).all()), "%s: written past the output" % tag


def call(name, *args):
    from ssl4gie_amd import _lib
    _lib.check(getattr(_lib.load(), name)(*args), name)


def on(c, *names):
    return [c[n].to(DEV).contiguous() for n in names]


# ------------------------------------------------------------------ the kernels, outputs as map_checks' evaluations name them
def run_bilinear(c, G):
    from ssl4gie_amd.ops import ptr, code, stream
    B, H, W, C = c["shape"]
    x, dy = on(c, "x", "dy")
    y, dx = G.out((B, 2 * H, 2 * W, C), c["dtype"]), G.out((B, H, W, C), c["dtype"])
    call("ssl4gie_bilinear2x_fwd", ptr(x), ptr(y), code(c["dtype"]), B, H, W, C, stream())
    call("ssl4gie_bilinear2x_bwd", ptr(dy), ptr(dx), code(c["dtype"]), B, H, W, C, stream())
    return {"y": y, "dx": dx}


def run_pool3(c, G):
    from ssl4gie_amd.ops import ptr, code, stream
    B, H, W, C = c["shape"]
    Ho, Wo = mc.out_hw(H, W)
    x, dy = on(c, "x", "dy")
    y, arg = G.out((B, Ho, Wo, C), c["dtype"]), G.out((B, Ho, Wo, C), torch.uint8)
    dx = G.out((B, H, W, C), c["dtype"])
    call("ssl4gie_maxpool3x3s2_fwd", ptr(x), ptr(y), ptr(arg), code(c["dtype"]), B, H, W, C, stream())
    call("ssl4gie_maxpool3x3s2_bwd", ptr(dy), ptr(arg), ptr(dx), code(c["dtype"]), B, H, W, C, stream())
    return {"y": y, "arg": arg, "dx": dx}


def run_pool2(c, G):
    from ssl4gie_amd.ops import ptr, code, stream
    B, H, W, C = c["shape"]
    x, dy = on(c, "x", "dy")
    y, dx = G.out((B, H // 2, W // 2, C), c["dtype"]), G.out((B, H, W, C), c["dtype"])
    call("ssl4gie_maxpool2x2_fwd", ptr(x), ptr(y), code(c["dtype"]), B, H, W, C, stream())
    call("ssl4gie_maxpool2x2_bwd", ptr(x), ptr(dy), ptr(dx), code(c["dtype"]), B, H, W, C, stream())
    return {"y": y, "dx": dx}


def run_avg(c, G):
    from ssl4gie_amd.ops import ptr, code, stream
    B, HW, C = c["shape"]
    x, dy = on(c, "x", "dy")
    y, dx = G.out((B, C), F32), G.out((B, HW, 1, C), c["dtype"])
    call("ssl4gie_avgpool_fwd", ptr(x), ptr(y), code(c["dtype"]), B, HW, C, stream())
    call("ssl4gie_avgpool_bwd", ptr(dy), ptr(dx), code(c["dtype"]), B, HW, C, stream())
    return {"y": y, "dx": dx}


def run_im2col(c, G):
    from ssl4gie_amd.ops import ptr, code, stream
    B, H, W, C = c["shape"]
    Ho, Wo = mc.out_hw(H, W, c["stride"])
    x, dcols = on(c, "x", "dcols")
    cols, dx = G.out((B * Ho * Wo, c["ld"]), c["dtype"]), G.out((B, H, W, C), c["dtype"])
    call("ssl4gie_im2col3x3", ptr(x), ptr(cols), code(c["dtype"]), B, H, W, C, c["stride"], c["relu"], c["ld"], stream())
    call("ssl4gie_col2im3x3", ptr(dcols), ptr(dx), code(c["dtype"]), B, H, W, C, c["stride"], c["ld"], stream())
    return {"cols": cols, "dx": dx}


def run_stem(c, G):
    from ssl4gie_amd.ops import ptr, code, stream
    B, H, W = c["shape"]
    Ho, Wo = mc.out_hw(H, W)
    img, = on(c, "img")
    cols = G.out((B * Ho * Wo, c["ld"]), c["dtype"])
    call("ssl4gie_stem_im2col7x7", ptr(img), ptr(cols), code(c["dtype"]), B, H, W, c["ld"], stream())
    return {"cols": cols}


def run_sub(c, G):
    from ssl4gie_amd.ops import ptr, code, stream
    B, H, W, C = c["shape"]
    Ho, Wo = mc.out_hw(H, W)
    x, dy = on(c, "x", "dy")
    y, dx = G.out((B, Ho, Wo, C), c["dtype"]), G.out((B, H, W, C), c["dtype"])
    call("ssl4gie_subsample2", ptr(x), ptr(y), code(c["dtype"]), B, H, W, C, 0, stream())
    call("ssl4gie_subsample2", ptr(dy), ptr(dx), code(c["dtype"]), B, H, W, C, 1, stream())
    return {"y": y, "dx": dx}


def run_shuffle(c, G):
    from ssl4gie_amd.ops import ptr, code, stream
    B, H, W, C = c["shape"]
    k = c["k"]
    g, bias = on(c, "g", "bias")
    y, yb = (G.out((B, k * H, k * W, C), c["dtype"]) for _ in range(2))
    dg = G.out((B * H * W, k * k * C), c["dtype"])
    call("ssl4gie_pixel_shuffle", ptr(g), 0, ptr(y), code(c["dtype"]), B, H, W, k, C, stream())
    call("ssl4gie_pixel_shuffle", ptr(g), ptr(bias), ptr(yb), code(c["dtype"]), B, H, W, k, C, stream())
    call("ssl4gie_pixel_unshuffle", ptr(y), ptr(dg), code(c["dtype"]), B, H, W, k, C, stream())
    return {"y": y, "yb": yb, "dg": dg}


def run_tokens(c, G):
    from ssl4gie_amd.ops import ptr, code, stream
    B, L, D = c["shape"]
    z, dx = on(c, "z", "dx")
    x, dz = G.out((B * L, D), c["dtype"]), G.out((B, L + 1, D), F32)
    call("ssl4gie_tokens_to_map", ptr(z), ptr(x), code(c["dtype"]), B, L, D, stream())
    call("ssl4gie_map_to_tokens", ptr(dx), ptr(dz), code(c["dtype"]), B, L, D, stream())
    return {"x": x, "dz": dz}


def run_eltwise(c, G):
    from ssl4gie_amd.ops import ptr, code, stream
    n, = c["shape"]
    a, b, s = on(c, "a", "b", "s")
    o = {k: G.out((n,), c["dtype"]) for k in ("add", "relu_bwd", "relu_bwd_skip", "gelu", "dgelu")}
    dt = code(c["dtype"])
    call("ssl4gie_eltwise", 0, ptr(a), ptr(b), 0, ptr(o["add"]), dt, n, stream())
    call("ssl4gie_eltwise", 1, ptr(a), ptr(b), 0, ptr(o["relu_bwd"]), dt, n, stream())
    call("ssl4gie_eltwise", 1, ptr(a), ptr(b), ptr(s), ptr(o["relu_bwd_skip"]), dt, n, stream())
    call("ssl4gie_gelu_map", ptr(a), 0, ptr(o["gelu"]), dt, n, stream())
    call("ssl4gie_gelu_map", ptr(a), ptr(b), ptr(o["dgelu"]), dt, n, stream())
    return o


def run_head(c, G, twice=False):
    from ssl4gie_amd import _lib
    from ssl4gie_amd.ops import ptr, code, stream
    M, C = c["shape"]
    x, w, bias, dy = on(c, "x", "w", "bias", "dy")
    acc = c["dw0"] is not None
    y, dx = G.out((M,), F32), G.out((M, C), c["dtype"])
    ws = torch.empty(max(16, _lib.load().ssl4gie_depth_head_bwd_workspace_bytes(M, C)), dtype=torch.uint8, device=DEV)
    call("ssl4gie_depth_head_fwd", ptr(x), ptr(w), ptr(bias), ptr(y), code(c["dtype"]), M, C, stream())
    res = []
    for _ in range(2 if twice else 1):
        dw, db = G.out((C,), F32, c["dw0"] if acc else None), G.out((1,), F32, c["db0"] if acc else None)
        call("ssl4gie_depth_head_bwd", ptr(x), ptr(w), ptr(y), ptr(dy), ptr(dx), ptr(dw), ptr(db), int(acc), ptr(ws),
             code(c["dtype"]), M, C, stream())
        res.append((dw, db))
    if twice:
        assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1]), "dw / db differ between two calls"
    return {"y": y, "dx": dx, "dw": res[0][0], "db": res[0][1]}


def run_ema(c, G):
    from ssl4gie_amd.ops import ptr, stream
    n, = c["shape"]
    src, = on(c, "src")
    out = G.out((n,), F32, c["dst"])
    call("ssl4gie_ema_update", ptr(out), ptr(src), float(c["m"]), n, stream())
    return {"out": out}


RUN = {"bilinear": run_bilinear, "pool3": run_pool3, "pool2": run_pool2, "avg": run_avg, "im2col": run_im2col,
       "stem": run_stem, "sub": run_sub, "shuffle": run_shuffle, "tokens": run_tokens, "eltwise": run_eltwise,
       "head": run_head, "ema": run_ema}
SPECS = {kind: mc.gpu_specs(kind) for kind in mc.KINDS}


def run_group(kind, group, **kw):
    rep = mc.Report()
    for grp, a in SPECS[kind]:
        if grp != group:
            continue
        c = mc.make(kind, a)
        tag = "%s %s %s" % (kind, group, a)
        G = Guard()
        o = RUN[kind](c, G, **kw)
        G.check(tag)
        rep.merge(mc.run_check(c, {k: v.cpu() for k, v in o.items()}, tag=tag))
    done(rep)


@pytest.mark.parametrize("group", mc.groups(SPECS["bilinear"]))
def test_bilinear2x_fwd_bwd(group):
    """1 x N and N x 1 maps (one axis with scale 0), the clamped last row and column of the 2 x 2-outputs-per-thread
    forward, more than one block per row (9 x 33 x 128)"""
    run_group("bilinear", group)


@pytest.mark.parametrize("group", mc.groups(SPECS["pool3"]))
def test_maxpool3x3s2_fwd_bwd(group):
    """the 16-byte kernels (C = V, 3V, 64) and the scalar ones (C not a whole chunk); odd and one-pixel maps"""
    run_group("pool3", group)


@pytest.mark.parametrize("group", mc.groups(SPECS["pool2"]))
def test_maxpool2x2_fwd_bwd(group):
    run_group("pool2", group)


@pytest.mark.parametrize("group", mc.groups(SPECS["avg"]))
def test_avgpool_fwd_bwd(group):
    run_group("avg", group)


@pytest.mark.parametrize("group", mc.groups(SPECS["im2col"]))
def test_im2col3x3_col2im3x3(group):
    """stride 1 and 2, ld = 9C, 9C + 24 and the GEMM's K padding; col2im ignores the pad columns (they hold noise)"""
    run_group("im2col", group)


@pytest.mark.parametrize("group", mc.groups(SPECS["stem"]))
def test_stem_im2col7x7(group):
    run_group("stem", group)


@pytest.mark.parametrize("group", mc.groups(SPECS["sub"]))
def test_subsample2_fwd_bwd(group):
    run_group("sub", group)


@pytest.mark.parametrize("group", mc.groups(SPECS["shuffle"]))
def test_pixel_shuffle_unshuffle(group):
    run_group("shuffle", group)


@pytest.mark.parametrize("group", mc.groups(SPECS["tokens"]))
def test_tokens_to_map_map_to_tokens(group):
    run_group("tokens", group)


@pytest.mark.parametrize("group", mc.groups(SPECS["eltwise"]))
def test_eltwise_add_relu_bwd_gelu_map(group):
    run_group("eltwise", group)


@pytest.mark.parametrize("group", mc.groups(SPECS["head"]))
def test_depth_head_fwd_bwd(group):
    """C = V, 32, 64 (the register array's limit); M = 1, 240, 257 and 262144 + 300 rows (the grid-stride loop);
    overwrite and accumulate into a pre-filled target; two calls give bit-equal dw and db"""
    run_group("head", group, twice=True)


@pytest.mark.parametrize("group", mc.groups(SPECS["ema"]))
def test_ema_update(group):
    """n % 4 != 0: the scalar tail, which arena slices never reach"""
    run_group("ema", group)


# ------------------------------------------------------------------ the fused BatchNorm (+ ReLU) pool
def _nan_to(t, v=12345.0):
    return torch.where(torch.isnan(t), torch.full_like(t, v), t)


@pytest.mark.parametrize("dtype", [F32, BF], ids=["fp32", "bf16"])
@pytest.mark.parametrize("family", ["quarter", "negative", "nan"])
def test_bn_maxpool_fused_equals_two_steps(dtype, family):
    """ssl4gie_bn_maxpool3x3s2_fwd against BatchNorm (+ ReLU) written out and pooled: values and arg bytes bit for bit,
    a NaN in the input included.  BatchNorm takes C % 8 == 0: C = 8, 24, 64"""
    from ssl4gie_amd import ops
    for (B, H, W) in mc.POOL3_MAPS:
        for C in (8, 24, 64):
            g = mc._gen(77, B, H, W, C)
            x = mc.fam("gauss" if family == "nan" else family, (B, H, W, C), g, dtype)
            if family == "nan":
                x.view(-1)[torch.randint(0, x.numel(), (1 + x.numel() // 50,), generator=g)] = float("nan")
            x = x.to(DEV)
            gamma, beta = torch.randn(C, generator=g).to(DEV), (0.3 * torch.randn(C, generator=g)).to(DEV)
            mean, rstd = (0.2 * torch.randn(C, generator=g)).to(DEV), (0.5 + torch.rand(C, generator=g)).to(DEV)
            coef = ops.bn_coef_stats(mean, rstd, gamma, beta)
            for relu in (True, False):
                y2 = ops.bn_fwd(x.view(-1, C), gamma, beta, None, None, None, 0.0, 1e-5, relu, False, mean, rstd)[0]
                y, arg = ops.maxpool3x3s2_fwd(y2.view(B, H, W, C))
                yf, argf = ops.maxpool3x3s2_fwd(x, coef, relu)
                tag = (family, B, H, W, C, relu)
                assert torch.equal(torch.isnan(yf), torch.isnan(y)), tag
                assert torch.equal(_nan_to(yf), _nan_to(y)) and torch.equal(argf, arg), tag
                if family == "nan":
                    assert bool(torch.isnan(yf).any()), tag
                else:       # and the two-step result is the reference's pool of the normalised map
                    yr, ar = mc.pool3_ref(y2.view(B, H, W, C).cpu())
                    assert torch.equal(yf.cpu(), yr) and torch.equal(argf.cpu(), ar), tag


# ------------------------------------------------------------------ NaN: ATen's `v > best || isnan(v)`
@pytest.mark.parametrize("dtype", [F32, BF], ids=["fp32", "bf16"])
@pytest.mark.parametrize("where", ["first", "middle", "last"])
def test_maxpool3x3s2_nan_follows_aten(dtype, where):
    """a single NaN at the first, a middle and the last position of window (1, 1) of a 5 x 5 map: it is the output of
    every window that holds it, the arg byte points at it and the backward routes those windows' gradients to it —
    F.max_pool2d on the CPU; the 16-byte kernels (C = V) and the scalar ones"""
    v = mc.V(dtype)
    iy, ix = {"first": (1, 1), "middle": (2, 2), "last": (3, 3)}[where]
    rep = mc.Report()
    for C in (v, v - 1):
        c = mc.pool3_case("gauss", 2, 5, 5, C, dtype, seed=3)
        c["x"][1, iy, ix, C - 1] = float("nan")
        G = Guard()
        o = {k: t.cpu() for k, t in run_pool3(c, G).items()}
        G.check("nan %s C %d" % (where, C))
        y, arg = mc.pool3_ref(c["x"])
        # rows / columns 1 and 3 belong to two windows each, row / column 2 to one
        assert int(torch.isnan(y).sum()) == {"first": 4, "middle": 1, "last": 4}[where] and bool(torch.isnan(y[1, 1, 1, C - 1]))
        assert torch.equal(torch.isnan(o["y"]), torch.isnan(y)), (where, C)
        rep.same("pool_y", _nan_to(o["y"]), _nan_to(y), "not the window's maximum")
        rep.same("pool_arg", o["arg"], arg, "the arg byte does not point at the NaN")
        dx, mag = mc.pool3_bwd(c["dy"], arg, 5, 5)
        rep.bounded("pool_dx", o["dx"], dx, mag)
        assert float(mag[1, iy, ix, C - 1]) > 0 and float(o["dx"][1, iy, ix, C - 1]) != 0
    done(rep)


@pytest.mark.parametrize("dtype", [F32, BF], ids=["fp32", "bf16"])
@pytest.mark.parametrize("t", [0, 1, 2, 3])
def test_maxpool2x2_nan_follows_aten(dtype, t):
    """a single NaN at each position of a 2 x 2 window: it is the output and receives the gradient"""
    C = mc.V(dtype)
    c = mc.pool2_case("gauss", 2, 4, 4, C, dtype, seed=5)
    c["x"][1, 2 + t // 2, 2 + t % 2, 1] = float("nan")
    G = Guard()
    o = {k: v.cpu() for k, v in run_pool2(c, G).items()}
    G.check("nan %d" % t)
    y, dx = mc.pool2_ref(c["x"], c["dy"])
    assert int(torch.isnan(y).sum()) == 1 and bool(torch.isnan(y[1, 1, 1, 1]))
    assert torch.equal(torch.isnan(o["y"]), torch.isnan(y))
    rep = mc.Report()
    rep.same("pool2_y", _nan_to(o["y"]), _nan_to(y), "not the window's maximum")
    rep.same("pool2_dx", o["dx"], dx, "the gradient does not go to the NaN")
    assert float(dx[1, 2 + t // 2, 2 + t % 2, 1]) == float(c["dy"][1, 1, 1, 1])
    done(rep)


# ------------------------------------------------------------------ what the interface refuses
def test_refusals_write_nothing():
    """maxpool2x2: odd H or W, C not a multiple of V; depth head: C = 72 — SSL4GIE_EARG from the library (the wrapper
    raises), nothing launched, nothing written"""
    from ssl4gie_amd import _lib, ops
    from ssl4gie_amd.ops import ptr, code, stream
    L = _lib.load()
    G = Guard()
    for dtype in (F32, BF):
        v = mc.V(dtype)
        for (H, W, C) in ((3, 4, v), (4, 3, v), (4, 4, v + 2), (4, 4, v // 2)):
            x = torch.ones(1, H, W, C, dtype=dtype, device=DEV)
            y, dx = G.out((1, 2, 2, 2 * v), dtype), G.out((1, 4, 4, 2 * v), dtype)
            assert L.ssl4gie_maxpool2x2_fwd(ptr(x), ptr(y), code(dtype), 1, H, W, C, stream()) == EARG
            assert L.ssl4gie_maxpool2x2_bwd(ptr(x), ptr(y), ptr(dx), code(dtype), 1, H, W, C, stream()) == EARG
            with pytest.raises(RuntimeError, match="invalid argument"):
                ops.maxpool2x2_fwd(x)
            assert bool((y == SENTINEL).all()) and bool((dx == SENTINEL).all())
        M, C = 16, 72
        x, w, b = torch.ones(M, C, dtype=dtype, device=DEV), torch.ones(C, device=DEV), torch.ones(1, device=DEV)
        y, dxh, dw, db = G.out((M,), F32), G.out((M, C), dtype), G.out((C,), F32), G.out((1,), F32)
        ws = torch.empty(1 << 16, dtype=torch.uint8, device=DEV)
        assert L.ssl4gie_depth_head_fwd(ptr(x), ptr(w), ptr(b), ptr(y), code(dtype), M, C, stream()) == EARG
        assert L.ssl4gie_depth_head_bwd(ptr(x), ptr(w), ptr(y), ptr(y), ptr(dxh), ptr(dw), ptr(db), 0, ptr(ws),
                                        code(dtype), M, C, stream()) == EARG
        with pytest.raises(RuntimeError, match="invalid argument"):
            ops.depth_head_fwd(x, w, b)
        for t in (y, dxh, dw, db):
            assert bool((t == SENTINEL).all())
    G.check("refusals")


def test_wrappers_agree_with_the_c_entry_points():
    """the ops wrappers (what the engines call) return what the guarded C calls returned: one case per kernel"""
    from ssl4gie_amd import ops
    eq = lambda a, b: a.dtype == b.dtype and a.shape == b.shape and torch.equal(a, b)
    for dtype in (F32, BF):
        v = mc.V(dtype)
        c = mc.bilinear_case("gauss", 2, 3, 5, 2 * v, dtype)
        o = run_bilinear(c, Guard())
        assert eq(ops.bilinear2x_fwd(c["x"].to(DEV)), o["y"]) and eq(ops.bilinear2x_bwd(c["dy"].to(DEV)), o["dx"])
        c = mc.pool3_case("quarter", 2, 7, 9, 3 * v, dtype)
        o = run_pool3(c, Guard())
        y, arg = ops.maxpool3x3s2_fwd(c["x"].to(DEV))
        assert eq(y, o["y"]) and eq(arg, o["arg"]) and eq(ops.maxpool3x3s2_bwd(c["dy"].to(DEV), arg, 7, 9), o["dx"])
        c = mc.im2col_case("signed_zero", 2, 7, 9, v, 2, mc.k_pad(9 * v, dtype), 1, dtype)
        o = run_im2col(c, Guard())
        assert ops.k_pad(9 * v, dtype) == c["ld"]
        assert eq(ops.im2col3x3(c["x"].to(DEV), 2, True), o["cols"])
        assert eq(ops.col2im3x3(c["dcols"].to(DEV), 2, 7, 9, v, 2), o["dx"])
        c = mc.stem_case(2, 7, 9, dtype)
        cols, Ho, Wo = ops.stem_im2col7x7(c["img"].to(DEV), dtype)
        assert (Ho, Wo) == (4, 5) and eq(cols, run_stem(c, Guard())["cols"])
        c = mc.head_case("gauss", 257, 32, dtype, True)
        o = run_head(c, Guard())
        x, w, b, dy = on(c, "x", "w", "bias", "dy")
        y = ops.depth_head_fwd(x, w, b)
        dw, db = c["dw0"].to(DEV), c["db0"].to(DEV)
        dx = ops.depth_head_bwd(x, w, y, dy, dw, db, True)
        assert eq(y, o["y"]) and eq(dx, o["dx"]) and eq(dw, o["dw"]) and eq(db, o["db"])
        c = mc.avg_case("gauss", 3, 49, 260, dtype)
        o = run_avg(c, Guard())
        assert eq(ops.avgpool_fwd(c["x"].to(DEV).view(3, 7, 7, 260)), o["y"])
        assert eq(ops.avgpool_bwd(c["dy"].to(DEV), 7, 7, dtype).view(3, 49, 1, 260), o["dx"])


def test_zz_worst_ratios():
    """not a check: the kernels' worst error / (2^-24 mag) per check over this module, for map_checks' table"""
    print("\nworst error / (2^-24 mag):", {n: float("%.3g" % v) for n, v in sorted(WORST.items()) if n in mc.BOUNDED})
