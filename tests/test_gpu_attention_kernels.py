"""Every variant behind ssl4gie_attn_fwd / ssl4gie_attn_bwd (csrc/attention.hip) against a plain fp64 reference, per
element (tests/attn_checks.py: the reference, the bounds and how their constants were derived; proof that the checks
bite: tests/test_attn_checks_cpu.py), through ssl4gie_amd.ops.

The case list puts a case on every branch of the dispatch:
  whole-head kernels   NKT = 2 ... 16 at the bucket's first N, the last half-tail N, the first N with one key in the
                       last tile and the full bucket (HT variants: forward at hd 32, backward at hd 64; AttnFwdQG and
                       U = 2 from NKT = 10 at hd 64, where the backward is the persistent prefetching kernel), `gauss`
                       at every scale; then EVERY N from 1 to 256 in the exact families `uniform` and `onehot`, where
                       a dropped, duplicated or leaked key or a fragment-layout slip cannot hide in the rounding;
  streaming kernels    the first block over the whole-head limit, one key and 127 keys in the last block, MASK and
                       no MASK, both head sizes;
  fp32 parity path     head sizes that are no multiple of 32 included;
  grid independence    a head's result must not depend on where in the grid it ran (xcd_remap at head counts that
                       are no multiple of 8; the persistent backward's walk);
  guard bands          every operand inside a larger allocation: the kernels neither read what is outside their
                       tensors (NaN margins) nor write it (sentinel margins);
  production heads     the batches the models run.
The ids say which branch a case is on."""
import math

import pytest
import torch

import attn_checks as ac

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32, BF, F64 = ac.F32, ac.BF, ac.F64
NAN_BITS = {BF: 0x7FC0, F32: 0x7FC00000}
SENTINEL = {BF: 0x5A5A, F32: 0x5A5A5A5A, torch.uint8: 0x5A}
INT_OF = {BF: torch.int16, F32: torch.int32, torch.uint8: torch.uint8}


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from ssl4gie_amd import _lib
    _lib.load()


def variant(N, hd):
    """which kernels (N, hd) takes on the bf16 path"""
    if N > 256:
        return "stream%s" % ("+MASK" if N % 128 else "")
    nkt = ac.nkt_of(N)
    half = N <= 16 * (nkt - 1)
    fwd = "fwd%s%s" % ("QG" if hd == 64 and nkt >= 10 else "", "+HT" if half and hd == 32 else "")
    pf = hd == 64 and nkt >= 10
    bwd = "bwd%s%s%s" % ("PF" if pf and ((N + 15) >> 4) >= nkt // 2 else "", "+U2" if pf else "",
                         "+HT" if half and hd == 64 else "")
    return "NKT%d-%s-%s" % (nkt, fwd, bwd)


def run(c):
    """forward and backward of case `c` (on the device) through ssl4gie_amd.ops; the backward is handed the
    forward's own stored O and lse, as the engine does"""
    from ssl4gie_amd import ops
    B, N, H, hd = c["B"], c["N"], c["H"], c["hd"]
    o, lse = ops.attn_fwd(c["qkv"], B, N, H, hd)
    dqkv = ops.attn_bwd(c["qkv"], o, c["do"], lse, B, N, H, hd)
    return o, lse, dqkv


def check_case(rep, family, B, N, H, hd, dtype, seed=0, **kw):
    c = ac.to_device(ac.make_case(family, B, N, H, hd, dtype, seed=seed, **kw), DEV)
    rep.tag = c["tag"] + (" " + variant(N, hd) if dtype == BF else "")
    o, lse, dqkv = run(c)
    ac.check_forward(rep, c, o, lse)
    ac.check_backward(rep, c, o, lse, dqkv)


def finish(rep):
    print("worst error beyond the u terms / (2^-24 mag):", {n: float("%.3g" % v) for n, v in sorted(rep.worst.items())})
    print("worst share of the u terms:", {n: float("%.3g" % v) for n, v in sorted(rep.worst_u.items())})
    rep.assert_ok()


def bucket_edges(nkt):
    return sorted({16 * (nkt - 2) + 1, 16 * (nkt - 1), 16 * (nkt - 1) + 1, 16 * nkt} | ({1} if nkt == 2 else set()))


# ===================================================================== whole-head kernels
@pytest.mark.parametrize("hd", [32, 64])
@pytest.mark.parametrize("nkt", range(2, 17, 2), ids=lambda n: "NKT%d" % n)
def test_whole_head_bucket_edges_gauss(nkt, hd):
    """each bucket at its first N, its last half-tail N, the first N with one key in the last tile, and full;
    random operands at scales 0.5, 1.5, 3 and with a per-head mean on q and k; every output per element"""
    rep = ac.Report()
    for N in bucket_edges(nkt):
        assert ac.nkt_of(N) == nkt
        for sc, off in ac.GAUSS_VARIANTS:
            check_case(rep, "gauss", 2, N, 3, hd, BF, seed=N, scale=sc, offset=off)
    finish(rep)


EXACT_FAMILIES = [("uniform", {"s0": s0}) for s0 in ac.UNIFORM_S0] + [("onehot", {})]


@pytest.mark.parametrize("hd", [32, 64])
@pytest.mark.parametrize("family,kw", EXACT_FAMILIES, ids=["uniform(0)", "uniform(-32)", "uniform(+32)", "onehot"])
def test_every_n_1_to_256_exact_families(family, kw, hd):
    """dense sweep, needs no knowledge of the tiling.  uniform: every score equal, V and dO small integers — lse is
    pinned at the 2^-24 level (one key too few or too many is a 1 / N error), and with the common score at -32 a
    zero-padded key that leaks takes over the softmax.  onehot: each query selects one key of a permutation — O is that
    V row and dV the permuted dO, exactly, and dQ = dK = 0"""
    rep = ac.Report()
    for N in range(1, 257):
        check_case(rep, family, 1, N, 2, hd, BF, seed=1, **kw)
    finish(rep)


# ===================================================================== streaming kernels
@pytest.mark.parametrize("hd", [32, 64])
@pytest.mark.parametrize("N", ac.STREAM_N, ids=lambda n: "N%d-%s" % (n, variant(n, 64)))
def test_streaming_kernels(N, hd):
    B, H = ac.stream_bh(N)
    rep = ac.Report()
    for sc, off in ac.GAUSS_VARIANTS:
        check_case(rep, "gauss", B, N, H, hd, BF, seed=2, scale=sc, offset=off)
    for s0 in ac.UNIFORM_S0:
        check_case(rep, "uniform", B, N, H, hd, BF, seed=2, s0=s0)
    if N <= 1024:
        check_case(rep, "onehot", B, N, H, hd, BF, seed=2)
    torch.cuda.empty_cache()
    finish(rep)


# ===================================================================== fp32 parity path
@pytest.mark.parametrize("hd", ac.FP32_HD)
@pytest.mark.parametrize("N", ac.FP32_N)
def test_fp32_parity_path(N, hd):
    """generic GEMMs + row softmax kernels: u = 0, every error is judged at the 2^-24 level"""
    rep = ac.Report()
    for sc, off in ac.GAUSS_VARIANTS:
        check_case(rep, "gauss", 2, N, 3, hd, F32, seed=4, scale=sc, offset=off)
    for s0 in ac.UNIFORM_S0:
        check_case(rep, "uniform", 2, N, 3, hd, F32, seed=4, s0=s0)
    finish(rep)


# ===================================================================== raw calls: pre-filled and guarded buffers
def bits(t):
    return t.view(INT_OF[t.dtype])


def filled(shape, dtype, pattern):
    t = torch.empty(shape, dtype=dtype, device=DEV)
    bits(t).fill_(pattern)
    return t


def raw_fwd(qkv, out, lse, B, N, H, hd, ws=None):
    from ssl4gie_amd import _lib, ops
    _lib.check(_lib.load().ssl4gie_attn_fwd(qkv.data_ptr(), out.data_ptr(), lse.data_ptr(), ops.code(qkv.dtype), B, N, H, hd,
                                            ops.ptr(ws), ops.stream()), "attn_fwd")


def raw_bwd(qkv, out, dout, lse, dqkv, B, N, H, hd, ws=None):
    from ssl4gie_amd import _lib, ops
    _lib.check(_lib.load().ssl4gie_attn_bwd(qkv.data_ptr(), out.data_ptr(), dout.data_ptr(), lse.data_ptr(), dqkv.data_ptr(),
                                            ops.code(qkv.dtype), B, N, H, hd, ops.ptr(ws), ops.stream()), "attn_bwd")


def workspace(dtype, B, N, H, hd):
    from ssl4gie_amd import _lib, ops
    return int(_lib.load().ssl4gie_attn_workspace_bytes(ops.code(dtype), B, N, H, hd))


def prefilled_run(qkv, do, B, N, H, hd):
    """forward + backward into outputs pre-filled with a NaN bit pattern -> (O, lse, dqkv)"""
    D = H * hd
    o, lse = filled((B, N, D), BF, NAN_BITS[BF]), filled((B, H, N), F32, NAN_BITS[F32])
    dqkv = filled(tuple(qkv.shape), BF, NAN_BITS[BF])
    nb = workspace(BF, B, N, H, hd)
    ws = filled((nb,), torch.uint8, 0xFF) if nb else None
    raw_fwd(qkv, o, lse, B, N, H, hd, ws)
    raw_bwd(qkv, o, do, lse, dqkv, B, N, H, hd, ws)
    return o, lse, dqkv


@pytest.mark.parametrize("hd", [64, 32])
@pytest.mark.parametrize("B,H", [(1, 1), (7, 1), (3, 3), (11, 3), (25, 10), (250, 1)],
                         ids=lambda v: str(v))
def test_grid_independence_forward_and_backward(B, H, hd):
    """B H = 1, 7, 9, 33, 250 heads (250 both as 25 x 10 and as 250 x 1) at N = 197: the whole batch in one launch
    equals each image in a launch of its own, bit for bit, forward (xcd_remap at head counts that are no multiple of
    8, the wave that takes the extra query tile rotating with the head) and backward (hd 64: the persistent
    prefetching kernel's walk against one head per workgroup).  Outputs are pre-filled with NaNs: an element nobody
    wrote fails the comparison."""
    N = 197
    c = ac.to_device(ac.make_case("gauss", B, N, H, hd, BF, seed=B * H, scale=1.5), DEV)
    o, lse, dqkv = prefilled_run(c["qkv"], c["do"], B, N, H, hd)
    for t, name in ((o, "O"), (lse, "lse"), (dqkv, "dqkv")):
        assert not bool(torch.isnan(t).any()), "%s: elements left unwritten (or NaN)" % name
    bad = []
    for b in range(B):
        o1, lse1, dqkv1 = prefilled_run(c["qkv"][b:b + 1].contiguous(), c["do"][b:b + 1].contiguous(), 1, N, H, hd)
        for got, one, name in ((o[b:b + 1], o1, "O"), (lse[b:b + 1], lse1, "lse"), (dqkv[b:b + 1], dqkv1, "dqkv")):
            if not torch.equal(bits(got.contiguous()), bits(one)):
                bad.append("image %d %s" % (b, name))
    assert not bad, bad[:20]
    rep = ac.Report()       # and the batch is right: first, middle and last image against fp64
    for b in sorted({0, B // 2, B - 1}):
        sub = dict(c, B=1, qkv=c["qkv"][b:b + 1], do=c["do"][b:b + 1])
        rep.tag = "%s image %d" % (c["tag"], b)
        ac.check_forward(rep, sub, o[b:b + 1], lse[b:b + 1])
        ac.check_backward(rep, sub, o[b:b + 1], lse[b:b + 1], dqkv[b:b + 1])
    finish(rep)


MARGIN = 4096       # elements on either side: a multiple of 16 bytes for every type, so the tensors keep their alignment


def guarded(shape, dtype, pattern, src=None):
    """a tensor of `shape` in the middle of a larger allocation filled with `pattern` -> (whole buffer, the tensor)"""
    n = math.prod(shape)
    buf = filled((n + 2 * MARGIN,), dtype, pattern)
    t = buf[MARGIN:MARGIN + n].view(shape)
    if src is not None:
        t.copy_(src)
    return buf, t


def margins_intact(buf, pattern):
    b = bits(buf)
    return bool((b[:MARGIN] == pattern).all()) and bool((b[-MARGIN:] == pattern).all())


@pytest.mark.parametrize("hd", [32, 64])
@pytest.mark.parametrize("N", [1, 17, 50, 193, 197, 209, 300], ids=lambda n: "N%d" % n)
def test_guard_bands(N, hd):
    """every operand sits inside its own larger allocation.  Inputs (qkv, O, dO, lse) between NaN margins: a tail load
    that runs past row N - 1 of the last image, or before the first, pulls a NaN into the result.  Outputs (O, lse,
    dqkv, the streaming backward's workspace) between sentinel margins: after the call the margins hold the sentinel,
    bit for bit, and the results equal those of the plain run, bit for bit."""
    B, H, D = 2, 3, 3 * hd
    c = ac.to_device(ac.make_case("gauss", B, N, H, hd, BF, seed=9, scale=1.5), DEV)
    o0, lse0, dqkv0 = run(c)
    nan16, nan32 = NAN_BITS[BF], NAN_BITS[F32]
    _, qkv = guarded(tuple(c["qkv"].shape), BF, nan16, c["qkv"])
    _, do = guarded((B, N, D), BF, nan16, c["do"])
    o_buf, o = guarded((B, N, D), BF, SENTINEL[BF])
    lse_buf, lse = guarded((B, H, N), F32, SENTINEL[F32])
    dq_buf, dqkv = guarded(tuple(c["qkv"].shape), BF, SENTINEL[BF])
    nb = workspace(BF, B, N, H, hd)
    ws_buf, ws = guarded((nb,), torch.uint8, SENTINEL[torch.uint8]) if nb else (None, None)
    raw_fwd(qkv, o, lse, B, N, H, hd, ws)
    torch.cuda.synchronize()
    assert margins_intact(o_buf, SENTINEL[BF]), "forward wrote outside O"
    assert margins_intact(lse_buf, SENTINEL[F32]), "forward wrote outside lse"
    assert torch.equal(bits(o), bits(o0)) and torch.equal(bits(lse), bits(lse0)), "forward differs from the plain run"
    # backward: the forward's results move between NaN margins as inputs
    _, o_in = guarded((B, N, D), BF, nan16, o)
    _, lse_in = guarded((B, H, N), F32, nan32, lse)
    raw_bwd(qkv, o_in, do, lse_in, dqkv, B, N, H, hd, ws)
    torch.cuda.synchronize()
    assert margins_intact(dq_buf, SENTINEL[BF]), "backward wrote outside dqkv"
    assert ws_buf is None or margins_intact(ws_buf, SENTINEL[torch.uint8]), "backward wrote outside its workspace"
    assert margins_intact(o_buf, SENTINEL[BF]) and margins_intact(lse_buf, SENTINEL[F32])
    assert torch.equal(bits(dqkv), bits(dqkv0)), "backward differs from the plain run"
    assert not bool(torch.isnan(dqkv).any()) and not bool(torch.isnan(o).any()) and not bool(torch.isnan(lse).any())


# ===================================================================== production heads
@pytest.mark.parametrize("B,N,H,hd", ac.PRODUCTION, ids=lambda v: str(v))
def test_production_heads(B, N, H, hd):
    """the batches the models run (MAE encoder, MAE decoder, ViT-B, MoCo vit_small, detection global attention), whole,
    random operands at scale 1.5; first, middle and last image against fp64"""
    c = ac.to_device(ac.make_case("gauss", B, N, H, hd, BF, seed=B + N, scale=1.5), DEV)
    o, lse, dqkv = run(c)
    rep = ac.Report()
    for b in sorted({0, B // 2, B - 1}):
        sub = dict(c, B=1, qkv=c["qkv"][b:b + 1], do=c["do"][b:b + 1])
        rep.tag = "%s %s image %d" % (c["tag"], variant(N, hd), b)
        ac.check_forward(rep, sub, o[b:b + 1], lse[b:b + 1])
        ac.check_backward(rep, sub, o[b:b + 1], lse[b:b + 1], dqkv[b:b + 1])
    del c, o, lse, dqkv
    torch.cuda.empty_cache()
    finish(rep)
