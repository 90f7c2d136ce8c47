"""The 13 kernels of mae_ops.hip — cast, cast_transpose, cast_transpose_batch, add_cast, mask_argsort, patch_gather,
tokens_assemble and its backward, strided_rowsum (dcls), decoder_assemble and its backward, mae_loss<1|3|4> and
normalize_u8 — against a plain fp64 reference, per element (tests/mae_checks.py: the references, the bounds, how
their constants were derived and the case list; tests/test_mae_checks_cpu.py: proof that the checks bite).

Every kernel is called through the C ABI with its outputs and workspaces in the middle of a buffer that carries 256
sentinel elements on either side (`Guard`) and is itself filled with the sentinel, so that a tail that writes past
the end and an element that is never written both show.  Both dtypes wherever an entry point takes one; the shapes
are the smallest at which each kernel can still go wrong (mae_checks.gpu_specs).

Run time on an MI355X: 115 tests in 3.3 s; the slowest after the first (which loads the library) is the
L = 16384 argsort at 0.11 s."""
import ctypes
import math

import pytest
import torch

import mae_checks as mk

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32, BF, F64, I64 = torch.float32, torch.bfloat16, torch.float64, torch.int64
EARG = 1000
SENTINEL, SENTINEL_BYTE, BAND = mk.SENTINEL, 0xAB, 256
WORST = {}      # worst error / (2^-24 mag) per check over the module (printed by the last test)
DENORMAL = {"rne": 0, "zero": 0}    # fp32 denormals the bf16 casts rounded / flushed


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from ssl4gie_amd import _lib
    _lib.load()


def done(rep):
    for n, v in rep.worst.items():
        WORST[n] = max(WORST.get(n, 0.0), v)
    for n, v in rep.denormal.items():
        DENORMAL[n] += v
    rep.assert_ok()


class Guard:
    """outputs with BAND sentinel elements before and after, themselves filled with the sentinel"""

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


def lib():
    from ssl4gie_amd import _lib
    return _lib.load()


def call(name, *args):
    from ssl4gie_amd import _lib
    _lib.check(getattr(_lib.load(), name)(*args), name)


def on(c, *names):
    return [None if c[n] is None else c[n].to(DEV).contiguous() for n in names]


def untouched(*ts):
    torch.cuda.synchronize()
    return all(bool((t == SENTINEL).all()) for t in ts)


# ------------------------------------------------------------------ the kernels, outputs as mae_checks' evaluations name them
def run_cast(c, G):
    from ssl4gie_amd.ops import ptr, code, stream
    n, = c["shape"]
    src, = on(c, "x")
    y = G.out((n,), c["dtype"])         # n = 0: an empty tensor has no address, both pointers are null
    call("ssl4gie_cast", ptr(src), ptr(y), code(c["dtype"]), n, stream())
    # the same into a slice that starts 64 elements into a larger buffer
    big = torch.full((n + 128,), SENTINEL, dtype=c["dtype"], device=DEV)
    call("ssl4gie_cast", ptr(src), ptr(big[64:]), code(c["dtype"]), n, stream())
    assert untouched(big[:64], big[64 + n:]), "cast into a slice wrote outside it"
    iv = torch.int16 if c["dtype"] == BF else torch.int32
    assert torch.equal(big[64:64 + n].view(iv), y.view(iv)), "cast into a slice differs"
    return {"y": y}


def run_transpose(c, G):
    from ssl4gie_amd.ops import ptr, code, stream
    rows, cols = c["shape"]
    x, = on(c, "x")
    y = G.out((cols, rows), c["dtype"])
    call("ssl4gie_cast_transpose", ptr(x), ptr(y), code(c["dtype"]), rows, cols, stream())
    return {"y": y}


def run_tbatch(c, G):
    from ssl4gie_amd.ops import ptr, stream
    x, = on(c, "x")
    off, rows, cols, ts, total = mk.tbatch_tables(c)
    off, rows, cols, ts = (t.to(DEV) for t in (off, rows, cols, ts))
    dst = G.out((c["total"],), BF)
    call("ssl4gie_cast_transpose_batch", ptr(x), ptr(dst), ptr(off), ptr(rows), ptr(cols), ptr(ts), len(c["shape"]),
         total, stream())
    return {"dst": dst}


def run_addcast(c, G):
    from ssl4gie_amd.ops import ptr, code, stream
    n, = c["shape"]
    a, b = on(c, "a", "b")
    out = G.out((n,), F32) if c["want_f32"] else None
    out_lp = G.out((n,), c["dtype"]) if c["dtype"] is not None else None
    call("ssl4gie_add_cast", ptr(a), ptr(b), ptr(out), ptr(out_lp), code(c["dtype"]) if c["dtype"] is not None else 0,
         n, stream())
    return {"out": out, "out_lp": out_lp}


def run_argsort(c, G):
    from ssl4gie_amd.ops import ptr, stream
    B, L = c["shape"]
    noise, = on(c, "noise")
    full = None
    for skip in (None, 0, 1, 2):        # all three outputs, then each pointer null in turn
        o = [None if i == skip else G.out((B, L), F32 if i == 2 else I64) for i in range(3)]
        call("ssl4gie_mask_argsort", ptr(noise), ptr(o[0]), ptr(o[1]), ptr(o[2]), B, L, c["len_keep"], stream())
        if full is None:
            full = o
        else:
            assert all(t is None or torch.equal(t, f) for t, f in zip(o, full)), "a null output pointer changes the others"
    return {"ids_shuffle": full[0], "ids_restore": full[1], "mask": full[2]}


def run_gather(c, G):
    from ssl4gie_amd.ops import ptr, code, stream
    B, C, H, W = c["shape"]
    img, ids = on(c, "img", "ids")
    out = G.out((B * c["nsel"], C * c["p"] ** 2), c["dtype"])
    call("ssl4gie_patch_gather", ptr(img), ptr(ids), ptr(out), code(c["dtype"]), B, C, H, W, c["p"], c["nsel"],
         0 if ids is None else ids.shape[1], c["order"], stream())
    return {"out": out}


def run_tokens(c, G):
    from ssl4gie_amd.ops import ptr, code, stream
    B, nsel, D = c["shape"]
    y, cls, pos, ids, dx = on(c, "y", "cls", "pos", "ids", "dx")
    x, dy = G.out((B, nsel + 1, D), F32), G.out((B * nsel, D), c["dtype"])
    call("ssl4gie_tokens_assemble", ptr(y), code(c["dtype"]), ptr(cls), ptr(pos), ptr(ids),
         0 if ids is None else ids.shape[1], ptr(x), B, nsel, D, stream())
    call("ssl4gie_tokens_assemble_bwd", ptr(dx), ptr(dy), code(c["dtype"]), 0, 0, B, nsel, D, stream())   # dcls null
    return {"x": x, "dy": dy}


def run_dcls(c, G):
    from ssl4gie_amd.ops import ptr, stream
    B, n1, D = c["shape"]
    dx, = on(c, "dx")
    dcls = G.out((D,), F32, c["init"])
    call("ssl4gie_tokens_assemble_bwd", ptr(dx), 0, 0, ptr(dcls), int(c["init"] is not None), B, n1 - 1, D, stream())
    return {"dcls": dcls}


def run_decoder(c, G):
    from ssl4gie_amd.ops import ptr, code, stream
    B, L, nkeep, D = c["shape"]
    y, mtok, dpos, dxd, s, r = on(c, "y", "mtok", "dpos", "dxd", "ids_shuffle", "ids_restore")
    xd, dy = G.out((B, L + 1, D), F32), G.out((B, nkeep + 1, D), c["dtype"])
    dm = G.out((D,), F32, c["init"])
    nws = lib().ssl4gie_decoder_assemble_bwd_workspace_bytes(B, L, D)
    assert nws == B * mk.DAB_Y * D * 4
    ws = G.out((nws // 4,), F32)
    call("ssl4gie_decoder_assemble", ptr(y), code(c["dtype"]), ptr(mtok), ptr(dpos), ptr(r), ptr(xd), B, L, nkeep, D,
         stream())
    call("ssl4gie_decoder_assemble_bwd", ptr(dxd), ptr(s), ptr(dy), code(c["dtype"]), ptr(dm), int(c["init"] is not None),
         ptr(ws), B, L, nkeep, D, stream())
    return {"xd": xd, "dy": dy, "dmask": dm}


def loss_call(c, has_cls, want_pp, want_dp, G):
    from ssl4gie_amd.ops import ptr, stream
    B, C, H, W = c["shape"]
    img, mask, gpp = on(c, "img", "mask", "gpp")
    pred = mk.loss_pred(c, has_cls).to(DEV)
    pp = G.out(tuple(mask.shape), F32) if want_pp else None
    dp = G.out(tuple(pred.shape), F32) if want_dp else None
    call("ssl4gie_mae_loss", ptr(pred), ptr(img), ptr(mask), ptr(pp), ptr(dp), ptr(gpp), float(c["gscale"]),
         c["norm_pix"], has_cls, B, C, H, W, c["p"], stream())
    return pp, dp


def run_loss(c, G):
    hc = c["has_cls"]
    pp, _ = loss_call(c, hc, True, False, G)
    pp2, dp = loss_call(c, hc, True, True, G)
    pp_alt, dp_alt = loss_call(c, 1 - hc, True, True, G)
    return {"pp": pp, "pp2": pp2, "dp": dp, "pp_alt": pp_alt, "dp_alt": dp_alt}


def c_floats(t):
    return (ctypes.c_float * 3)(*[float(v) for v in t])


def run_u8(c, G):
    from ssl4gie_amd.ops import ptr, stream
    B, H, W = c["shape"]
    img, = on(c, "img")
    out = G.out((B, 3, H, W), F32)
    call("ssl4gie_normalize_u8", ptr(img), ptr(out), c_floats(c["mean"]), c_floats(c["std"]), B, H, W, stream())
    return {"out": out}


RUN = {"cast": run_cast, "transpose": run_transpose, "tbatch": run_tbatch, "addcast": run_addcast, "argsort": run_argsort,
       "gather": run_gather, "tokens": run_tokens, "dcls": run_dcls, "decoder": run_decoder, "loss": run_loss,
       "u8": run_u8}
SPECS = {kind: mk.gpu_specs(kind) for kind in mk.KINDS}


def run_case(kind, c, tag):
    G = Guard()
    o = RUN[kind](c, G)
    G.check(tag)
    return mk.run_check(c, {k: None if v is None else v.cpu() for k, v in o.items()}, tag=tag)


def run_group(kind, group):
    rep = mk.Report()
    for grp, a in SPECS[kind]:
        if grp == group:
            rep.merge(run_case(kind, mk.make(kind, a), "%s %s %s" % (kind, group, a)))
    done(rep)


@pytest.mark.parametrize("group", mk.groups(SPECS["cast"]))
def test_cast(group):
    """n = 0, below one vector, n % 4 != 0, either side of one block, 1024 k + 3; the specials (NaN, +-0, +-inf, RNE
    ties, denormals, 0x7f7fffff); also into a slice 64 elements into a larger buffer"""
    run_group("cast", group)


@pytest.mark.parametrize("group", mk.groups(SPECS["transpose"]))
def test_cast_transpose(group):
    """1 x n, n x 1, one short of a tile, a tile, ragged edges both ways"""
    run_group("transpose", group)


@pytest.mark.parametrize("group", mk.groups(SPECS["tbatch"]))
def test_cast_transpose_batch(group):
    """seven matrices of one arena in one launch (vector and scalar paths, ragged tiles, 1 x n, n x 1), and one
    alone; the gaps of dst keep the sentinel"""
    run_group("tbatch", group)


@pytest.mark.parametrize("group", mk.groups(SPECS["addcast"]))
def test_add_cast(group):
    run_group("addcast", group)


@pytest.mark.parametrize("group", mk.groups(SPECS["argsort"]))
def test_mask_argsort(group):
    """L = 1 .. 1024 on either side of the wave and of the 256-thread stride, len_keep 0, 1, L // 4, L, ties and
    zeros of either sign; every output pointer null in turn"""
    run_group("argsort", group)


def test_mask_argsort_at_the_documented_limit():
    """L = 16384: 64 KiB of dynamic LDS, one block"""
    done(run_case("argsort", mk.argsort_case("uniform", 1, mk.ARGSORT_MAX_L, mk.ARGSORT_MAX_L // 4), "argsort L 16384"))


@pytest.mark.parametrize("group", mk.groups(SPECS["gather"]))
def test_patch_gather(group):
    """H != W, p = 4 (most of the block idle), p = 32 (more than one sweep), C = 1, 3, 4, both column orders, ids
    rows wider than nsel"""
    run_group("gather", group)


@pytest.mark.parametrize("group", mk.groups(SPECS["tokens"]))
def test_tokens_assemble_fwd_bwd(group):
    """D = 4 .. 1028 (one 64-thread block, exactly one sweep of 256 threads, a second sweep), bf16 y, ids rows wider
    than nsel; the backward with dcls null"""
    run_group("tokens", group)


@pytest.mark.parametrize("group", mk.groups(SPECS["dcls"]))
def test_tokens_assemble_bwd_dcls(group):
    """strided_rowsum_kernel: B below, at and above the 16 row groups, D not a multiple of 64, accumulate; dy null"""
    run_group("dcls", group)


@pytest.mark.parametrize("group", mk.groups(SPECS["decoder"]))
def test_decoder_assemble_fwd_bwd(group):
    """nkeep = 0 and L, fewer removed rows than row groups, a second sweep over D, bf16, accumulate"""
    run_group("decoder", group)


@pytest.mark.parametrize("group", mk.groups(SPECS["loss"]))
def test_mae_loss(group):
    """NV = 1, 3, 4, a partly filled last slot (P = 48, 320, 588), H != W, row counts that are no multiple of 4,
    the three masks, gpp given and None, gscale 1 and 0.125, constant patches under norm_pix"""
    run_group("loss", group)


@pytest.mark.parametrize("group", mk.groups(SPECS["u8"]))
def test_normalize_u8(group):
    run_group("u8", group)


# ------------------------------------------------------------------ determinism
def test_reductions_are_deterministic():
    """dcls, dmask and per_patch are bit-equal between two runs"""
    for kind, a, name in (("dcls", ("gauss", 40, 132, 1), "dcls"),
                          ("decoder", ("gauss", 2, 20, 1, 1028, F32, 1), "dmask"),
                          ("loss", ("offset", 3, 3, 64, 64, 16, 1, 1, "random", 1, 0.125), "pp")):
        c = mk.make(kind, a)
        first, second = RUN[kind](c, Guard())[name], RUN[kind](c, Guard())[name]
        assert torch.equal(first.view(torch.int32), second.view(torch.int32)), kind


# ------------------------------------------------------------------ what the interface refuses
def test_refusals_write_nothing():
    """SSL4GIE_EARG from the library (the wrapper raises), nothing launched, nothing written; B = 0 returns 0 and
    writes nothing.  patch_gather's W % 4 != 0 cannot be reached on its own: p % 4 == 0 and W % p == 0 imply it"""
    from ssl4gie_amd import ops
    from ssl4gie_amd.ops import ptr, stream
    L = lib()
    G = Guard()
    dev = lambda *s: torch.ones(*s, device=DEV)
    raises = lambda: pytest.raises(RuntimeError, match="invalid argument")
    out = G.out((4096,), F32)
    out2 = G.out((4096,), F32)
    # patch_gather: (B, C, H, W, p, nsel, order)
    for (B, C, H, W, p, nsel, order) in ((1, 3, 28, 28, 14, 4, 0), (1, 3, 20, 16, 16, 1, 0), (1, 1, 6, 6, 6, 1, 0),
                                          (1, 1, 16, 18, 16, 1, 0), (1, 1, 8, 8, 4, 5, 0), (1, 1, 8, 8, 4, 4, 2)):
        assert L.ssl4gie_patch_gather(ptr(dev(B, C, H, W)), 0, ptr(out), 0, B, C, H, W, p, nsel, 0, order, stream()) == EARG
    with raises():
        ops.patch_gather(dev(1, 3, 28, 28), 14)
    with raises():
        ops.patch_gather(dev(1, 1, 8, 8), 4, order=2)
    assert L.ssl4gie_patch_gather(ptr(dev(1, 1, 8, 8)), 0, ptr(out), 0, 0, 1, 8, 8, 4, 4, 0, 0, stream()) == 0
    # add_cast
    a = dev(8)
    assert L.ssl4gie_add_cast(ptr(a), 0, ptr(out), ptr(out2), 0, 6, stream()) == EARG
    assert L.ssl4gie_add_cast(ptr(a), 0, 0, 0, 0, 8, stream()) == EARG
    with raises():
        ops.add_cast(dev(6))
    with raises():
        ops.add_cast(dev(8), want_f32=False)
    # mask_argsort
    noise = dev(1, 64)
    iout = G.out((4096,), I64)
    for (B, Ln, keep) in ((1, 0, 0), (1, mk.ARGSORT_MAX_L + 1, 1), (1, 64, 65)):
        assert L.ssl4gie_mask_argsort(ptr(noise), ptr(iout), ptr(iout), ptr(out), B, Ln, keep, stream()) == EARG
    with raises():
        ops.mask_argsort(noise, 65)
    assert L.ssl4gie_mask_argsort(ptr(noise), ptr(iout), ptr(iout), ptr(out), 0, 64, 16, stream()) == 0
    # mae_loss: P = 1028 and P % 4 != 0
    for (C, p) in ((257, 2), (1, 3)):
        img, pred, mask = dev(1, C, 2 * p, 2 * p), dev(1, 4, C * p * p), dev(1, 4)
        assert L.ssl4gie_mae_loss(ptr(pred), ptr(img), ptr(mask), ptr(out), ptr(out2), 0, 1.0, 0, 0, 1, C, 2 * p, 2 * p,
                                  p, stream()) == EARG
        with raises():
            ops.mae_loss_fwd(pred, img, mask, p, False)
        with raises():
            ops.mae_loss_bwd(pred, img, mask, p, False, None)
    img, pred, mask = dev(1, 3, 8, 8), dev(1, 4, 48), dev(1, 4)
    assert L.ssl4gie_mae_loss(ptr(pred), ptr(img), ptr(mask), ptr(out), ptr(out2), 0, 1.0, 0, 0, 0, 3, 8, 8, 4, stream()) == 0
    # normalize_u8
    u8 = torch.zeros(1, 3, 3, 3, dtype=torch.uint8, device=DEV)
    m, s = c_floats(mk.IMAGENET[0]), c_floats(mk.IMAGENET[1])
    assert L.ssl4gie_normalize_u8(ptr(u8), ptr(out), m, s, 1, 3, 3, stream()) == EARG           # H W % 4 != 0
    assert L.ssl4gie_normalize_u8(ptr(u8), ptr(out), m, c_floats((0.2, 0.0, 0.2)), 1, 1, 4, stream()) == EARG
    with raises():
        ops.normalize_u8(u8)
    with raises():
        ops.normalize_u8(torch.zeros(1, 1, 4, 3, dtype=torch.uint8, device=DEV), std=(0.2, 0.0, 0.2))
    # tokens_assemble / decoder_assemble: D % 4 != 0, nkeep > L, an unknown dtype code
    y, cls, pos, dx = dev(4, 8), dev(8), dev(8, 8), dev(2, 3, 8)
    for (D, dt) in ((6, 0), (8, 7)):
        assert L.ssl4gie_tokens_assemble(ptr(y), dt, ptr(cls), ptr(pos), 0, 0, ptr(out), 2, 2, D, stream()) == EARG
        assert L.ssl4gie_tokens_assemble_bwd(ptr(dx), ptr(out), dt, ptr(out2), 0, 2, 2, D, stream()) == EARG
    with raises():
        ops.tokens_assemble(dev(4, 6), dev(6), dev(8, 6), 2, 2)
    with raises():
        ops.tokens_assemble_bwd(dev(2, 3, 6), F32)
    assert L.ssl4gie_tokens_assemble(ptr(y), 0, ptr(cls), ptr(pos), 0, 0, ptr(out), 0, 2, 8, stream()) == 0
    assert L.ssl4gie_tokens_assemble_bwd(ptr(dx), ptr(out), 0, ptr(out2), 0, 0, 2, 8, stream()) == 0
    r = torch.zeros(2, 4, dtype=I64, device=DEV)
    yd, mt, dpos, dxd, ws = dev(2, 5, 8), dev(8), dev(5, 8), dev(2, 5, 8), G.out((4096,), F32)
    for (nkeep, D, dt) in ((5, 8, 0), (2, 6, 0), (2, 8, 7)):
        assert L.ssl4gie_decoder_assemble(ptr(yd), dt, ptr(mt), ptr(dpos), ptr(r), ptr(out), 2, 4, nkeep, D, stream()) == EARG
        assert L.ssl4gie_decoder_assemble_bwd(ptr(dxd), ptr(r), ptr(out), dt, ptr(out2), 0, ptr(ws), 2, 4, nkeep, D,
                                              stream()) == EARG
    with raises():
        ops.decoder_assemble(dev(2, 3, 6), dev(6), dev(5, 6), r, 2)
    with raises():
        ops.decoder_assemble_bwd(dev(2, 5, 6), r, 2, F32, dev(6))
    assert L.ssl4gie_decoder_assemble(ptr(yd), 0, ptr(mt), ptr(dpos), ptr(r), ptr(out), 0, 4, 2, 8, stream()) == 0
    assert L.ssl4gie_decoder_assemble_bwd(ptr(dxd), ptr(r), ptr(out), 0, ptr(out2), 0, ptr(ws), 0, 4, 2, 8, stream()) == 0
    assert untouched(out, out2, ws) and bool((iout == int(SENTINEL)).all())
    G.check("refusals")


def test_wrappers_agree_with_the_c_entry_points():
    """the ops wrappers (what the engines call) return what the guarded C calls returned: one case per wrapper,
    cast(..., out=slice) and cast_transpose(..., out=...) as engine.py calls them included"""
    from ssl4gie_amd import ops

    def eq(a, b):
        iv = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[a.element_size()]
        return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().view(iv), b.contiguous().view(iv))
    for dtype in (F32, BF):
        c = mk.cast_case("specials", 1025, dtype)
        o = run_cast(c, Guard())
        x = c["x"].to(DEV)
        assert eq(ops.cast(x, dtype), o["y"])
        big = torch.full((1025 + 128,), SENTINEL, dtype=dtype, device=DEV)
        assert eq(ops.cast(x, dtype, out=big[64:64 + 1025]), o["y"]) and untouched(big[:64], big[64 + 1025:])
        c = mk.transpose_case("gauss", 45, 70, dtype)
        o = run_transpose(c, Guard())
        assert eq(ops.cast_transpose(c["x"].to(DEV), dtype), o["y"])
        big = torch.full((45 * 70 + 128,), SENTINEL, dtype=dtype, device=DEV)
        assert eq(ops.cast_transpose(c["x"].to(DEV), dtype, out=big[64:64 + 45 * 70]).view(70, 45), o["y"])
        assert untouched(big[:64], big[64 + 45 * 70:])
        c = mk.addcast_case("gauss", 1028, 1, 1, dtype)
        o = run_addcast(c, Guard())
        out, out_lp = ops.add_cast(c["a"].to(DEV), c["b"].to(DEV), True, dtype)
        assert eq(out, o["out"]) and eq(out_lp, o["out_lp"])
        c = mk.gather_case("signed_zero", 2, 3, 32, 48, 16, 1, 1, dtype)
        o = run_gather(c, Guard())
        assert eq(ops.patch_gather(c["img"].to(DEV), 16, c["ids"].to(DEV), c["nsel"], dtype, 1), o["out"])
        c = mk.tokens_case("signed_zero", 2, 5, 252, dtype, 1)
        o = run_tokens(c, Guard())
        y, cls, pos, ids, dx = on(c, "y", "cls", "pos", "ids", "dx")
        assert eq(ops.tokens_assemble(y, cls, pos, 2, 5, ids), o["x"])
        d = mk.dcls_case("gauss", 2, 252, 1)
        d["dx"], d["shape"] = c["dx"], tuple(c["dx"].shape)
        dcls = d["init"].to(DEV)
        assert eq(ops.tokens_assemble_bwd(dx, dtype, dcls, True), o["dy"]) and eq(dcls, run_dcls(d, Guard())["dcls"])
        c = mk.decoder_case("gauss", 2, 12, 9, 8, dtype, 1)
        o = run_decoder(c, Guard())
        y, mtok, dpos, dxd, s, r = on(c, "y", "mtok", "dpos", "dxd", "ids_shuffle", "ids_restore")
        assert eq(ops.decoder_assemble(y, mtok, dpos, r, 9), o["xd"])
        dm = c["init"].to(DEV)
        assert eq(ops.decoder_assemble_bwd(dxd, s, 9, dtype, dm, True), o["dy"]) and eq(dm, o["dmask"])
    c = mk.argsort_case("ties", 3, 257, 64)
    o = run_argsort(c, Guard())
    s, r, m = ops.mask_argsort(c["noise"].to(DEV), 64)
    assert eq(s, o["ids_shuffle"]) and eq(r, o["ids_restore"]) and eq(m, o["mask"])
    for hc in (0, 1):
        c = mk.loss_case("gauss", 3, 3, 64, 64, 16, 1, hc, "random", 1, 0.125)
        o = run_loss(c, Guard())
        pred, img, mask, gpp = mk.loss_pred(c, hc).to(DEV), c["img"].to(DEV), c["mask"].to(DEV), c["gpp"].to(DEV)
        assert eq(ops.mae_loss_fwd(pred, img, mask, 16, True), o["pp"])
        assert eq(ops.mae_loss_bwd(pred, img, mask, 16, True, gpp, 0.125), o["dp"])
    for identity in (0, 1):
        c = mk.u8_case(3, 30, 28, identity)
        o = run_u8(c, Guard())
        kw = {"mean": mk.IDENTITY[0], "std": mk.IDENTITY[1]} if identity else {}
        assert eq(ops.normalize_u8(c["img"].to(DEV), **kw), o["out"])


def test_zz_worst_ratios():
    """the kernels' worst error / (2^-24 mag) per check over this module, for mae_checks' table, and what became of
    the fp32 denormals in the bf16 casts; every check of mae_checks was exercised at least once"""
    print("\nworst error / (2^-24 mag):", {n: float("%.3g" % v) for n, v in sorted(WORST.items()) if n in mk.BOUNDED})
    print("fp32 denormals cast to bf16:", DENORMAL)
    missing = (set(mk.BOUNDED) | set(mk.EXACT)) - set(WORST)
    assert not missing, "never exercised: %s" % sorted(missing)
