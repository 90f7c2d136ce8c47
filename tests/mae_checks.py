"""fp64 references of the MAE glue, cast and loss kernels of mae_ops.hip (casts and transposes, add_cast, the integer
masking, patch gather, encoder / decoder token assembly and their backward, the MAE loss and its gradient, the uint8
normalisation) and the per-element checks that pin those kernels to them (tests/test_gpu_mae_kernels.py; proof that
the checks bite: tests/test_mae_checks_cpu.py).

References: plain torch on the CPU, in float64 wherever anything is added or multiplied, starting from exactly the
bits the kernel is handed (a bf16 input is rounded first and the reference sees the rounded value; mean / std of the
normalisation and gscale are taken as rounded to fp32).
    cast, cast_transpose(_batch)   x.to(dt), x.t().contiguous().to(dt) of CPU torch (RNE)
    add_cast                       the fp32 a + b of CPU torch (a alone without b); out_lp = that value rounded
    mask_argsort                   ids_shuffle = torch.argsort(noise, dim=1, stable=True), ids_restore = its inverse
                                   permutation, mask[i] = rank(i) >= len_keep.  -0.0 and +0.0 compare equal (a tie, the
                                   index decides).  NaN noise is out of scope: torch.rand never produces it, and the
                                   counting rank of a NaN (it is neither below nor equal to anything) is no permutation.
    patch_gather                   order 0: the rows of F.unfold(img, p, stride=p); order 1: the nchpwq -> nhwpqc
                                   patchify; with ids the rows ids[b, :nsel]
    tokens_assemble                [cls + pos[0] | y[b, j] + pos[1 + patch(b, j)]] in fp32;  bwd: dy = dx[:, 1:],
                                   dcls = sum_b dx[b, 0]
    decoder_assemble               [y[b, 0] | y[b, 1 + r] if r < nkeep else mask_token] + dpos, r = ids_restore;
                                   bwd: dy = [dxd[b, 0] | dxd[b, 1 + ids_shuffle[b, j]], j < nkeep],
                                   dmask = sum over b and j >= nkeep of dxd[b, 1 + ids_shuffle[b, j]]
    mae_loss                       t = patchify(img) ('nhwpqc'); norm_pix: that = (t - mean) (var_unbiased + 1e-6)^-1/2;
                                   per_patch = m mean_k (pred - that)^2, dpred = gscale gpp m 2 / P (pred - that)
    normalize_u8                   (x / 255 - mean[c]) / std[c], HWC -> CHW

Two kinds of check, per output element, never a global norm.
  Bit for bit (`Report.same` of map_checks: dtype, shape and the BITS): every output that is a copy, a selection, a
  cast, or one correctly rounded fp32 addition followed by at most one RNE rounding — cast, cast_t, cast_tb (the
  sentinel between the matrices of the arena included), add_cast, add_cast_lp, ids_shuffle, ids_restore, mask, gather,
  tok_fwd, tok_bwd, dec_fwd, dec_bwd; of the loss: the cls row of dpred is +0 (loss_cls_row), dpred is 0 wherever the
  mask is 0 (loss_masked, either sign: it is a product with m = 0), per_patch of a forward-only call is per_patch of
  the call that also returns dpred (loss_pp_same), and pred laid out as [B, L, P] or [B, 1 + L, P] gives the same
  bits for the same patches (loss_layout).  With the `integers` family every sum is exact, so dcls, dmask and
  per_patch without norm_pix equal the fp64 value rounded once (the reference asserts its sums stay below 2^24).
  The casts (`Report.same_cast`): NaN positions compare as NaN on both sides, not by payload.  An fp32 denormal
  going to bf16 may arrive as the RNE result or as a zero of the same sign; the MI355X gave the RNE result at every
  such position (v_cvt_pk_bf16_f32 does not flush: tests/test_gpu_mae_kernels.py counts both and printed
  rne = all, zero = 0), as CPU torch does.  An fp32 -> fp32 cast is a copy and keeps a denormal's bits.
  Bounded: |got - ref| <= u |ref| + k 2^-24 mag, u = 2^-8 for a bf16 output and 0 otherwise, mag = the fp64 sum of
  the ABSOLUTE values of the terms the kernel adds:
    dcls      sum_b |dx[b, 0, d]|  (+ |initial| with accumulate)
    dmask     sum over the removed rows of all samples |dxd|  (+ |initial|)
    loss_pp   m mean_k (d_k^2 + 2 |d_k| delta_k), d = pred - that: each square rounds at its own size and the sum at
              no more than the sum of squares; an error e of that_k moves d_k^2 by 2 |d_k| e
    loss_dp   |gs| (|pred| + |that| + delta), gs = gscale gpp m 2 / P
    norm_u8   |x / (255 std)| + |mean / std|: the kernel multiplies by a rounded reciprocal (two roundings of the
              scale, one of the shift, one multiply-add), so it is not bit-equal to (x / 255 - mean) / std
  delta, the size of that's own error: 0 without norm_pix (the target is a pixel, copied).  With norm_pix
    delta = r (|t| + mean |t|) + |t - mu| (r^3 / 2 var + r),  r = (var + 1e-6)^-1/2, var over P - 1:
  the mean is a sum about 0 (error mean |t|) and t - mean rounds at |t|, both multiplied by r; r itself is off by
  (r^3 / 2) times the error of var (which rounds at its own size) plus its own rounding — the y and rstd reasoning of
  ln_checks.  The first term is what a constant patch needs: var = 0, r = 10^3, and an fp32 mean that is off by one
  ulp of |t| shows in that at 10^3 times its size — r |t| charges exactly that, so the `const` and `offset`
  families need no larger k.

k.  Procedure (as in bn_checks / attn_checks / ln_checks / map_checks): evaluate the same formulae in plain fp32 torch
(`EVAL`, neither the library nor the engine: `sum()` reductions, `var()`, `rsqrt`), run it through these checks
over the case list of the GPU module (`measure_k_ref`), record the worst error / (2^-24 mag) per check as k_ref — the
larger of torch on the CPU and torch on the MI355X — and set k = max(16, 4 k_ref) rounded up to a power of two.
The kernels' column is what tests/test_gpu_mae_kernels.py printed on an MI355X (its last test).

    check      k_ref CPU  k_ref MI355X  k     kernels' worst ratio
    dcls           1.69         1.66    16     1.69
    dmask          1.81         1.98    16     1.88
    loss_pp        2.83         2.78    16     2.55
    loss_dp        3.16         3.16    16     2.56
    norm_u8        1.13         1.66    16     1.66

Input families (generated on the CPU from fixed seeds):
    gauss        N(0, 1)
    integers     in [-4, 4] (pred, gpp, the initial values too): every sum is exact
    offset       100 + N(0, 1): an image mean of 100 sigma, the variance cancels
    const        every patch of the image constant, a multiple of 1/4 in [-8, 8]: its sum is exact, its variance 0
    tiny         1e-3 N(0, 1): a patch variance of the size of the 1e-6 under the root (where that 1e-6 sits shows)
    signed_zero  N(0, 1) with +0.0 and -0.0 at a quarter of the positions each
    uniform      torch.rand (the masking noise);  ties: noise from the 4 levels {0, 1/4, 1/2, 3/4} with the zeros of
                 either sign, the first row all equal;  signed_zero (noise): rand with +0.0 / -0.0 at a quarter each
    specials     the casts only: +-0, +-inf, NaN (quiet and signalling payloads), the smallest normal, the largest and
                 smallest denormals, denormals bf16 can hold and a denormal tie, 0x7f7fffff (rounds to bf16 inf), and
                 for an even and an odd bit 16 the fp32 words whose low half is 0x7fff, 0x8000 and 0x8001, both signs
"""
import math

import torch
import torch.nn.functional as Fn

import map_checks as mc
from ln_checks import EPS32, F64, F32, BF, k_from, u_of      # noqa: F401
from map_checks import _gen, dname

BOUNDED = ("dcls", "dmask", "loss_pp", "loss_dp", "norm_u8")
EXACT = ("cast", "cast_t", "cast_tb", "add_cast", "add_cast_lp", "ids_shuffle", "ids_restore", "mask", "gather",
         "tok_fwd", "tok_bwd", "dec_fwd", "dec_bwd", "loss_cls_row", "loss_masked", "loss_pp_same", "loss_layout")
CHECKS = BOUNDED
# worst error / (2^-24 mag) of the fp32 torch evaluation over the GPU module's case list (measure_k_ref)
K_REF_CPU = {"dcls": 1.692, "dmask": 1.810, "loss_pp": 2.832, "loss_dp": 3.159, "norm_u8": 1.127}
K_REF_GPU = {"dcls": 1.657, "dmask": 1.976, "loss_pp": 2.778, "loss_dp": 3.159, "norm_u8": 1.656}
K_REF = {n: max(K_REF_CPU.get(n, 0.0), K_REF_GPU.get(n, 0.0)) for n in CHECKS}
K = {name: k_from(v) for name, v in K_REF.items()}
SENTINEL = 12288.0          # what the GPU module fills outputs and guard bands with (a bf16 value)
DAB_Y = 8                   # mae_ops.hip: row groups of decoder_assemble_bwd_kernel
ARGSORT_MAX_L = 16384       # ssl4gie_hip.h: 64 KiB of dynamic LDS
LOSS_MAX_P = 1024

_SPECIAL_WORDS = [0x00000000, 0x80000000, 0x7f800000, 0xff800000, 0x7fc00000, 0xffc00000, 0x7f800001, 0x7fc12345,
                  0x00800000, 0x80800000, 0x007fffff, 0x807fffff, 0x00000001, 0x80000001, 0x00010000, 0x80010000,
                  0x00018000, 0x00008000, 0x80008000, 0x00008001, 0x7f7fffff, 0xff7fffff,
                  0x3f807fff, 0x3f808000, 0x3f808001, 0x3f817fff, 0x3f818000, 0x3f818001,
                  0xbf807fff, 0xbf808000, 0xbf808001, 0xbf817fff, 0xbf818000, 0xbf818001]


def specials(n):
    w = torch.tensor([v - (1 << 32) if v >= (1 << 31) else v for v in _SPECIAL_WORDS], dtype=torch.int32)
    return w.repeat(n // len(w) + 1)[:n].contiguous().view(F32)


def is_denormal(x):
    b = x.contiguous().view(torch.int32)
    return ((b & 0x7f800000) == 0) & ((b & 0x007fffff) != 0)


class Report(mc.Report):
    def __init__(self, tag="", measure=False, k=None):
        super().__init__(tag, measure, K if k is None else k)
        self.denormal = {"rne": 0, "zero": 0}

    def same_cast(self, name, got, x, what="not x rounded to nearest even"):
        """got against x.to(got.dtype) of CPU torch: NaN positions as NaN, an fp32 denormal going to bf16 as the
        RNE result or a zero of its sign (counted in self.denormal), everything else by its bits"""
        want = x.to(got.dtype)
        if self.measure or got.dtype != want.dtype or got.shape != want.shape:
            return self.same(name, got, want, what)
        nan = torch.isnan(want)
        if not torch.equal(torch.isnan(got), nan):
            self.worst[name] = math.inf
            self.failed.append("%s %s: the NaN positions differ" % (self.tag, name))
            return
        g, w = torch.where(nan, torch.zeros_like(got), got), torch.where(nan, torch.zeros_like(want), want)
        if got.dtype == BF:
            den = is_denormal(x)
            zero = torch.where(torch.signbit(x), -torch.zeros_like(w), torch.zeros_like(w))
            iv = lambda t: t.contiguous().view(torch.int16)
            flushed = den & (iv(g) == iv(zero)) & (iv(w) != iv(zero))
            self.denormal["zero"] += int(flushed.sum())
            self.denormal["rne"] += int((den & ~flushed & (iv(g) == iv(w)) & (iv(w) != iv(zero))).sum())
            w = torch.where(flushed, zero, w)
        self.same(name, g, w, what)

    def merge(self, other):
        for n, v in getattr(other, "denormal", {}).items():
            self.denormal[n] += v
        return super().merge(other)


# ------------------------------------------------------------------ inputs
FAMILIES = ("gauss", "integers", "offset", "const", "signed_zero", "uniform", "ties", "specials", "tiny")


def fam(family, shape, g, dtype=F32):
    shape = tuple(shape)
    if family == "offset":
        return (100.0 + torch.randn(shape, generator=g)).to(dtype)
    if family == "tiny":
        return (1e-3 * torch.randn(shape, generator=g)).to(dtype)
    if family == "specials":
        return specials(math.prod(shape)).view(shape).to(dtype)
    return mc.fam(family, shape, g, dtype)


def _key(family, dtype, *dims):
    return (FAMILIES.index(family), {None: 2, BF: 1, F32: 0}[dtype]) + tuple(int(d) for d in dims)


def _dev(c):
    return c.get("device", "cpu")


def _t(c, name, dt=None):
    t = c[name]
    return None if t is None else t.to(device=_dev(c)) if dt is None else t.to(device=_dev(c), dtype=dt)


def _cpu(o):
    return {k: (v.cpu() if torch.is_tensor(v) else v) for k, v in o.items()}


def _truncate_bf16(t):
    return (t.contiguous().view(torch.int32) & -65536).view(F32).to(BF)


def perm_rows(B, L, g):
    return torch.stack([torch.randperm(L, generator=g) for _ in range(B)]).contiguous()


# ===================================================================== cast
def cast_case(family, n, dtype, seed=0):
    g = _gen(21, seed, *_key(family, dtype, n))
    return {"kind": "cast", "family": family, "dtype": dtype, "shape": (n,), "x": fam(family, (n,), g)}


def cast_eval(c, mut=None):
    x, dt = _t(c, "x"), c["dtype"]
    y = _truncate_bf16(x) if mut == "cast_truncated" and dt == BF else x.to(dt)
    n = x.numel()
    if mut == "cast_tail_dropped" and n % 4:
        y[n - n % 4:] = 0
    return _cpu({"y": y})


def cast_check(c, o, rep):
    rep.same_cast("cast", o["y"], c["x"])


# ===================================================================== cast_transpose
def transpose_case(family, rows, cols, dtype, seed=0):
    g = _gen(22, seed, *_key(family, dtype, rows, cols))
    return {"kind": "transpose", "family": family, "dtype": dtype, "shape": (rows, cols),
            "x": fam(family, (rows, cols), g)}


def transpose_eval(c, mut=None):
    rows, cols = c["shape"]
    x = _t(c, "x")
    y = x.t().contiguous().to(c["dtype"])
    if mut == "transpose_edge_swapped":        # the guard r < rows && c < cols read as r < cols && c < rows
        r, cc = torch.arange(rows, device=x.device).view(1, -1), torch.arange(cols, device=x.device).view(-1, 1)
        y = torch.where((r < cols) & (cc < rows), y, torch.zeros_like(y))
    return _cpu({"y": y})


def transpose_check(c, o, rep):
    rep.same_cast("cast_t", o["y"], c["x"].t().contiguous(), "not the transpose rounded to nearest even")


# ===================================================================== cast_transpose_batch
def tbatch_case(mats, seed=0):
    """matrices at 64-element aligned offsets of one fp32 arena, at least 64 elements apart"""
    g = _gen(23, seed, len(mats), *[d for m in mats for d in m])
    off, at = [], 64
    for r, cc in mats:
        off.append(at)
        at = (at + r * cc + 63) // 64 * 64 + 64
    return {"kind": "tbatch", "family": "gauss", "dtype": BF, "shape": tuple(mats), "off": off, "total": at,
            "x": torch.randn(at, generator=g)}


def tbatch_tables(c):
    """(mat_off int64 [S], rows int32 [S], cols int32 [S], tile_start int32 [S + 1], total tiles)"""
    ts = [0]
    for r, cc in c["shape"]:
        ts.append(ts[-1] + ((r + 63) // 64) * ((cc + 63) // 64))
    return (torch.tensor(c["off"], dtype=torch.int64), torch.tensor([m[0] for m in c["shape"]], dtype=torch.int32),
            torch.tensor([m[1] for m in c["shape"]], dtype=torch.int32), torch.tensor(ts, dtype=torch.int32), ts[-1])


def _tbatch(c, x, swapped=False):
    dst = torch.full((c["total"],), SENTINEL, dtype=BF, device=x.device)
    for (r, cc), o in zip(c["shape"], c["off"]):
        y = x[o:o + r * cc].view(r, cc).t().contiguous().to(BF)
        if swapped:
            ri, ci = torch.arange(r, device=x.device).view(1, -1), torch.arange(cc, device=x.device).view(-1, 1)
            y = torch.where((ri < cc) & (ci < r), y, torch.zeros_like(y))
        dst[o:o + r * cc] = y.reshape(-1)
    return dst


def tbatch_eval(c, mut=None):
    return _cpu({"dst": _tbatch(c, _t(c, "x"), mut == "transpose_edge_swapped")})


def tbatch_check(c, o, rep):
    rep.same("cast_tb", o["dst"], _tbatch(c, c["x"]), "not the bf16 transposes at their offsets, the sentinel between")


# ===================================================================== add_cast
def addcast_case(family, n, has_b, want_f32, lp, seed=0):
    g = _gen(24, seed, *_key(family, lp, n, has_b, want_f32))
    return {"kind": "addcast", "family": family, "dtype": lp, "shape": (n,), "want_f32": bool(want_f32),
            "a": fam(family, (n,), g), "b": fam(family, (n,), g) if has_b else None}


def addcast_eval(c, mut=None):
    a, b = _t(c, "a"), _t(c, "b")
    s = a if b is None else a + b
    return _cpu({"out": s if c["want_f32"] else None, "out_lp": None if c["dtype"] is None else s.to(c["dtype"])})


def addcast_check(c, o, rep):
    s = c["a"] if c["b"] is None else c["a"] + c["b"]
    if c["want_f32"]:
        rep.same("add_cast", o["out"], s, "not the fp32 a + b")
    if c["dtype"] is not None:
        rep.same("add_cast_lp", o["out_lp"], s.to(c["dtype"]), "not a + b rounded to the operand type")


# ===================================================================== mask_argsort
def noise_of(family, B, L, g):
    if family == "uniform":
        return torch.rand(B, L, generator=g)
    if family == "ties":
        x = torch.randint(0, 4, (B, L), generator=g).float() / 4
        x = torch.where((x == 0) & (torch.rand(B, L, generator=g) < 0.5), torch.tensor(-0.0), x)
        x[0] = 0.5
        return x
    x = torch.rand(B, L, generator=g)
    r = torch.randint(0, 4, (B, L), generator=g)
    x = torch.where(r == 0, torch.tensor(0.0), x)
    return torch.where(r == 1, torch.tensor(-0.0), x)


def argsort_case(family, B, L, len_keep, seed=0):
    g = _gen(25, seed, *_key(family, F32, B, L))
    return {"kind": "argsort", "family": family, "dtype": F32, "shape": (B, L), "len_keep": len_keep,
            "noise": noise_of(family, B, L, g)}


def masking(noise, len_keep, unstable=False, gt=False):
    """(ids_shuffle, ids_restore, mask) of a [B, L] noise"""
    B, L = noise.shape
    if unstable:        # equal values in descending index order
        ids = L - 1 - torch.argsort(noise.flip(1), dim=1, stable=True)
    else:
        ids = torch.argsort(noise, dim=1, stable=True)
    restore = torch.empty_like(ids).scatter_(1, ids, torch.arange(L, device=noise.device).expand(B, L).contiguous())
    mask = ((restore > len_keep) if gt else (restore >= len_keep)).to(F32)
    return ids, restore, mask


def argsort_eval(c, mut=None):
    s, r, m = masking(_t(c, "noise"), c["len_keep"], mut == "argsort_unstable", mut == "mask_gt")
    return _cpu({"ids_shuffle": s, "ids_restore": r, "mask": m})


def argsort_check(c, o, rep):
    s, r, m = masking(c["noise"], c["len_keep"])
    rep.same("ids_shuffle", o["ids_shuffle"], s, "not the stable ascending argsort")
    rep.same("ids_restore", o["ids_restore"], r, "not the rank")
    rep.same("mask", o["mask"], m, "not rank >= len_keep")


# ===================================================================== patch_gather
def gather_case(family, B, C, H, W, p, order, with_ids, dtype, seed=0):
    g = _gen(26, seed, *_key(family, dtype, B, C, H, W, p, order, with_ids))
    n = (H // p) * (W // p)
    return {"kind": "gather", "family": family, "dtype": dtype, "shape": (B, C, H, W), "p": p, "order": order,
            "img": fam(family, (B, C, H, W), g), "ids": perm_rows(B, n, g) if with_ids else None,
            "nsel": max(1, 3 * n // 4) if with_ids else n}


def patches_by_index(img, p, order):
    """[B, gh * gw, P] written out by index: order 0 columns (c, py, px), order 1 columns (py, px, c)"""
    B, C, H, W = img.shape
    v = img.reshape(B, C, H // p, p, W // p, p)
    v = v.permute(0, 2, 4, 1, 3, 5) if order == 0 else v.permute(0, 2, 4, 3, 5, 1)
    return v.reshape(B, (H // p) * (W // p), C * p * p)


def _selection(c, ids, mut, dev):
    """patch index [B, nsel] the kernel reads"""
    B, nsel = c["shape"][0], c["nsel"]
    if ids is None:
        return torch.arange(nsel, device=dev).expand(B, nsel)
    if mut in ("ids_stride_nsel", "gather_ids_stride_nsel"):
        return ids.reshape(-1)[:B * nsel].view(B, nsel)
    return ids[:, :nsel]


def gather_eval(c, mut=None):
    B, C, H, W = c["shape"]
    p, gh, gw = c["p"], c["shape"][2] // c["p"], c["shape"][3] // c["p"]
    img, ids = _t(c, "img"), _t(c, "ids")
    order = 1 - c["order"] if mut == "gather_column_order" else c["order"]
    sel = _selection(c, ids, mut, img.device)
    if mut == "gather_gw_from_H":
        sel = ((sel // gh) % gh) * gw + (sel % gh) % gw
    allp = patches_by_index(img, p, order)
    out = torch.gather(allp, 1, sel[:, :, None].expand(B, c["nsel"], allp.shape[2]))
    return _cpu({"out": out.reshape(B * c["nsel"], -1).to(c["dtype"])})


def gather_ref(c):
    B, C, H, W = c["shape"]
    p = c["p"]
    if c["order"] == 0:
        allp = Fn.unfold(c["img"], p, stride=p).transpose(1, 2)
    else:
        allp = c["img"].reshape(B, C, H // p, p, W // p, p)
        allp = torch.einsum("nchpwq->nhwpqc", allp).reshape(B, (H // p) * (W // p), p * p * C)
    if c["ids"] is not None:
        allp = torch.stack([allp[b, c["ids"][b, :c["nsel"]]] for b in range(B)])
    return allp.reshape(B * c["nsel"], C * p * p).to(c["dtype"])


def gather_check(c, o, rep):
    rep.same("gather", o["out"], gather_ref(c), "not the selected patch rows")


# ===================================================================== tokens_assemble / _bwd (dy)
def tokens_case(family, B, nsel, D, dtype, with_ids, seed=0):
    g = _gen(27, seed, *_key(family, dtype, B, nsel, D, with_ids))
    L = nsel + 3 if with_ids else nsel
    return {"kind": "tokens", "family": family, "dtype": dtype, "shape": (B, nsel, D), "nsel": nsel, "L": L,
            "y": fam(family, (B * nsel, D), g, dtype), "cls": fam(family, (D,), g), "pos": fam(family, (1 + L, D), g),
            "ids": perm_rows(B, L, g) if with_ids else None, "dx": fam(family, (B, nsel + 1, D), g)}


def tokens_eval(c, mut=None, dt=F32):
    B, nsel, D = c["shape"]
    y, cls, pos, dx, ids = _t(c, "y", dt), _t(c, "cls", dt), _t(c, "pos", dt), _t(c, "dx", dt), _t(c, "ids")
    sel = _selection(c, ids, mut, y.device)
    rows = pos[sel if mut == "pos_patch_not_shifted" else 1 + sel]
    x = torch.cat([(cls + pos[0]).view(1, 1, D).expand(B, 1, D), y.view(B, nsel, D) + rows], 1)
    return _cpu({"x": x.float(), "dy": dx[:, 1:].reshape(B * nsel, D).to(c["dtype"])})


def tokens_check(c, o, rep):
    B, nsel, D = c["shape"]
    sel = _selection(c, c["ids"], None, "cpu")
    want = torch.cat([(c["cls"] + c["pos"][0]).view(1, 1, D).expand(B, 1, D),
                      c["y"].float().view(B, nsel, D) + c["pos"][1 + sel]], 1)
    rep.same("tok_fwd", o["x"], want, "not [cls + pos[0] | y + pos[1 + patch]] in fp32")
    rep.same("tok_bwd", o["dy"], c["dx"][:, 1:].reshape(B * nsel, D).to(c["dtype"]), "not dx[:, 1:] in the operand type")


# ===================================================================== tokens_assemble_bwd (dcls)
def _init(family, D, g, accumulate):
    if not accumulate:
        return None
    return torch.randint(-4, 5, (D,), generator=g).float() if family == "integers" else torch.randn(D, generator=g)


def dcls_case(family, B, D, accumulate, seed=0):
    g = _gen(28, seed, *_key(family, F32, B, D, accumulate))
    return {"kind": "dcls", "family": family, "dtype": F32, "shape": (B, 3, D), "dx": fam(family, (B, 3, D), g),
            "init": _init(family, D, g, accumulate)}


def dcls_eval(c, mut=None, dt=F32):
    dx, init = _t(c, "dx", dt), _t(c, "init", dt)
    B = dx.shape[0]
    s = dx[:B // 16 * 16 if mut == "dcls_rows_multiple_of_16" else B, 0].sum(0)
    if init is not None and mut != "accumulate_ignored":
        s = s + init
    return _cpu({"dcls": s.float()})


def _summed(rows, init, integers):
    """fp64 sum over dim 0 of rows [n, D] (+ init), the mag of its bound"""
    s, t = rows.to(F64).sum(0), rows.to(F64).abs().sum(0)
    if init is not None:
        s, t = s + init.to(F64), t + init.to(F64).abs()
    if integers:
        assert float(t.max()) < 2 ** 24, "the integer sums must stay exact in fp32"
    return s, t


def dcls_check(c, o, rep):
    s, t = _summed(c["dx"][:, 0], c["init"], c["family"] == "integers")
    rep.bounded("dcls", o["dcls"], s, t, exact=c["family"] == "integers")


# ===================================================================== decoder_assemble / _bwd
def decoder_case(family, B, L, nkeep, D, dtype, accumulate, seed=0):
    g = _gen(29, seed, *_key(family, dtype, B, L, nkeep, D, accumulate))
    s, r, _ = masking(torch.rand(B, L, generator=g), nkeep)
    return {"kind": "decoder", "family": family, "dtype": dtype, "shape": (B, L, nkeep, D), "ids_shuffle": s,
            "ids_restore": r, "y": fam(family, (B, nkeep + 1, D), g, dtype), "mtok": fam(family, (D,), g),
            "dpos": fam(family, (L + 1, D), g), "dxd": fam(family, (B, L + 1, D), g),
            "init": _init(family, D, g, accumulate)}


def _rows(t, idx):
    """t [B, n, D] at idx [B, m] -> [B, m, D]"""
    return torch.gather(t, 1, idx[:, :, None].expand(idx.shape[0], idx.shape[1], t.shape[2]))


def decoder_eval(c, mut=None, dt=F32):
    B, L, nkeep, D = c["shape"]
    y, mtok, dpos, dxd, init = (_t(c, n, dt) for n in ("y", "mtok", "dpos", "dxd", "init"))
    s, r = _t(c, "ids_shuffle"), _t(c, "ids_restore")
    beyond = torch.full((B, 1, D), float("nan"), dtype=dt, device=y.device)     # what lies behind y's kept rows
    src = torch.cat([y[:, 1:], beyond if mut == "dec_r_le_nkeep" else mtok.view(1, 1, D).expand(B, 1, D),
                     mtok.view(1, 1, D).expand(B, L, D)], 1)[:, :L + 1]
    first = y[:, min(1, nkeep):min(1, nkeep) + 1] if mut == "dec_cls_from_row_1" else y[:, :1]
    xd = torch.cat([first, _rows(src, r)], 1) + dpos
    dy = torch.cat([dxd[:, :1], _rows(dxd[:, 1:], s[:, :nkeep])], 1).to(c["dtype"])
    gone = _rows(dxd[:, 1:], s[:, nkeep:])
    if mut == "dmask_rows_beyond_8_dropped":
        gone = gone[:, :DAB_Y]
    dm = gone.sum((0, 1))
    if init is not None and mut != "dmask_accumulate_ignored":
        dm = dm + init
    return _cpu({"xd": xd.float(), "dy": dy, "dmask": dm.float()})


def decoder_check(c, o, rep):
    B, L, nkeep, D = c["shape"]
    s, r = c["ids_shuffle"], c["ids_restore"]
    src = torch.cat([c["y"][:, 1:].float(), c["mtok"].view(1, 1, D).expand(B, L - nkeep, D)], 1)
    rep.same("dec_fwd", o["xd"], torch.cat([c["y"][:, :1].float(), _rows(src, r)], 1) + c["dpos"],
             "not [y[b, 0] | kept row or mask token] + dpos in fp32")
    rep.same("dec_bwd", o["dy"], torch.cat([c["dxd"][:, :1], _rows(c["dxd"][:, 1:], s[:, :nkeep])], 1).to(c["dtype"]),
             "not [dxd[b, 0] | the kept rows] in the operand type")
    ref, mag = _summed(_rows(c["dxd"][:, 1:], s[:, nkeep:]).reshape(-1, D), c["init"], c["family"] == "integers")
    rep.bounded("dmask", o["dmask"], ref, mag, exact=c["family"] == "integers" or nkeep == L)


# ===================================================================== mae_loss
MASKS = ("random", "zeros", "ones")


def loss_case(family, B, C, H, W, p, norm_pix, has_cls, mask, with_gpp, gscale, seed=0):
    g = _gen(30, seed, *_key(family, F32, B, C, H, W, p, norm_pix, has_cls, MASKS.index(mask), with_gpp, gscale * 1000))
    gh, gw = H // p, W // p
    L, P = gh * gw, C * p * p
    if family == "const":
        v = torch.randint(-32, 33, (B, 1, gh, 1, gw, 1), generator=g).float() / 4
        img = v.expand(B, C, gh, p, gw, p).reshape(B, C, H, W).contiguous()
    else:
        img = fam(family, (B, C, H, W), g)
    other = "integers" if family == "integers" else "gauss"
    m = {"random": (torch.rand(B, L, generator=g) > 0.3).float(), "zeros": torch.zeros(B, L), "ones": torch.ones(B, L)}
    return {"kind": "loss", "family": family, "dtype": F32, "shape": (B, C, H, W), "p": p, "norm_pix": norm_pix,
            "has_cls": has_cls, "gscale": gscale, "img": img, "pred": fam(other, (B, L + 1, P), g), "mask": m[mask],
            "gpp": fam(other, (B, L), g) if with_gpp else None}


def loss_pred(c, has_cls):
    """pred as handed to the kernel: [B, 1 + L, P], or the same patch rows as [B, L, P]"""
    return c["pred"] if has_cls else c["pred"][:, 1:].contiguous()


def loss_eval(c, mut=None, dt=F32):
    B, C, H, W = c["shape"]
    p, P = c["p"], C * c["p"] ** 2
    img, pred, m, gpp = _t(c, "img", dt), _t(c, "pred", dt), _t(c, "mask", dt), _t(c, "gpp", dt)
    t = patches_by_index(img, p, 1)
    if mut == "loss_gw_from_H":
        gh, gw = H // p, W // p
        l = torch.arange(gh * gw, device=img.device)
        t = t[:, ((l // gh) % gh) * gw + (l % gh) % gw]
    if c["norm_pix"]:
        mean = t.mean(-1, keepdim=True)
        var = t.var(-1, keepdim=True, unbiased=mut != "loss_biased_var")
        t = (t - mean) / (var.sqrt() + 1e-6) if mut == "loss_eps_outside_root" else (t - mean) * torch.rsqrt(var + 1e-6)
    d = pred[:, 1:] - t
    pp = (d * d).mean(-1) * m
    gs = torch.full_like(m, 1.0 if mut == "loss_gscale_ignored" else c["gscale"])
    if gpp is not None and mut != "loss_gpp_ignored":
        gs = gs * gpp
    if mut != "loss_dpred_not_masked":
        gs = gs * m
    gs = gs * (1.0 if mut == "loss_no_2_over_P" else 2.0 / P)
    dp = d * gs[:, :, None]
    first = pred[:, :1] * 0.5 if mut == "loss_cls_row_nonzero" else torch.zeros_like(pred[:, :1])
    with_cls = torch.cat([first, dp], 1)
    a, b = (with_cls, dp) if c["has_cls"] else (dp, with_cls)
    return _cpu({"pp": pp.float(), "pp2": pp.float(), "dp": a.float(), "pp_alt": pp.float(), "dp_alt": b.float()})


def loss_ref(c):
    """fp64: per_patch, dpred of the patch rows, and the mags of their bounds"""
    B, C, H, W = c["shape"]
    p, P = c["p"], C * c["p"] ** 2
    t = torch.einsum("nchpwq->nhwpqc", c["img"].to(F64).reshape(B, C, H // p, p, W // p, p)).reshape(B, -1, P)
    delta = torch.zeros_like(t)
    if c["norm_pix"]:
        mu, var = t.mean(-1, keepdim=True), t.var(-1, keepdim=True)
        r = (var + 1.0e-6) ** -0.5
        delta = r * (t.abs() + t.abs().mean(-1, keepdim=True)) + (t - mu).abs() * (0.5 * r ** 3 * var + r)
        t = (t - mu) * r
    pred, m = c["pred"][:, 1:].to(F64), c["mask"].to(F64)
    d = pred - t
    gs = float(torch.tensor(c["gscale"], dtype=F32)) * m * 2.0 / P
    if c["gpp"] is not None:
        gs = gs * c["gpp"].to(F64)
    gs = gs[:, :, None]
    if c["family"] == "integers" and not c["norm_pix"]:
        assert float((d * d).sum(-1).max()) < 2 ** 24, "the integer sums must stay exact in fp32"
    return {"pp": (d * d).mean(-1) * m, "t_pp": (d * d + 2 * d.abs() * delta).mean(-1) * m,
            "dp": gs * d, "t_dp": gs.abs() * (pred.abs() + t.abs() + delta)}


def loss_check(c, o, rep):
    r, hc = loss_ref(c), c["has_cls"]
    rep.bounded("loss_pp", o["pp"], r["pp"], r["t_pp"], exact=c["family"] == "integers" and not c["norm_pix"])
    rep.bounded("loss_dp", o["dp"][:, hc:], r["dp"], r["t_dp"])
    with_cls = o["dp"] if hc else o["dp_alt"]
    rep.same("loss_cls_row", with_cls[:, 0], torch.zeros_like(with_cls[:, 0]), "the cls row of dpred is not +0")
    off = (c["mask"] == 0)[:, :, None].expand_as(r["dp"])
    rep.same("loss_masked", torch.where(off, o["dp"][:, hc:], torch.zeros(())).abs(), torch.zeros_like(o["dp"][:, hc:]),
             "dpred is not 0 where the mask is 0")
    rep.same("loss_pp_same", o["pp2"], o["pp"], "per_patch differs between the forward-only and the forward + gradient call")
    rep.same("loss_layout", o["pp_alt"], o["pp"], "per_patch differs between pred [B, L, P] and [B, 1 + L, P]")
    rep.same("loss_layout", o["dp_alt"][:, 1 - hc:], o["dp"][:, hc:], "dpred differs between pred [B, L, P] and [B, 1 + L, P]")


# ===================================================================== normalize_u8
IMAGENET = ((0.485, 0.456, 0.406), (0.229, 0.224, 0.225))
IDENTITY = ((0.0, 0.0, 0.0), (1.0, 1.0, 1.0))


def u8_case(B, H, W, identity, seed=0):
    g = _gen(31, seed, B, H, W, identity)
    n = B * H * W * 3
    if n < 256:
        v = torch.linspace(0, 255, n).round()
    else:
        v = torch.cat([torch.arange(256.0), torch.randint(0, 256, (n - 256,), generator=g).float()])
    mean, std = IDENTITY if identity else IMAGENET
    return {"kind": "u8", "family": "bytes", "dtype": F32, "shape": (B, H, W), "mean": torch.tensor(mean),
            "std": torch.tensor(std), "img": v[torch.randperm(n, generator=g)].to(torch.uint8).view(B, H, W, 3)}


def u8_eval(c, mut=None, dt=F32):
    x = _t(c, "img").permute(0, 3, 1, 2).to(dt)
    mean, std = _t(c, "mean", dt).view(1, 3, 1, 1), _t(c, "std", dt).view(1, 3, 1, 1)
    if mut == "u8_channels_swapped":
        x = x.flip(1)
    return _cpu({"out": ((x / (256.0 if mut == "u8_div_256" else 255.0) - mean) / std).float().contiguous()})


def u8_check(c, o, rep):
    x = c["img"].permute(0, 3, 1, 2).to(F64)
    mean, std = c["mean"].to(F64).view(1, 3, 1, 1), c["std"].to(F64).view(1, 3, 1, 1)
    rep.bounded("norm_u8", o["out"], (x / 255 - mean) / std, (x / (255 * std)).abs() + (mean / std).abs().expand_as(x))


# ===================================================================== table
# kind -> (case constructor, fp32 evaluation, check)
KINDS = {"cast": (cast_case, cast_eval, cast_check), "transpose": (transpose_case, transpose_eval, transpose_check),
         "tbatch": (tbatch_case, tbatch_eval, tbatch_check), "addcast": (addcast_case, addcast_eval, addcast_check),
         "argsort": (argsort_case, argsort_eval, argsort_check), "gather": (gather_case, gather_eval, gather_check),
         "tokens": (tokens_case, tokens_eval, tokens_check), "dcls": (dcls_case, dcls_eval, dcls_check),
         "decoder": (decoder_case, decoder_eval, decoder_check), "loss": (loss_case, loss_eval, loss_check),
         "u8": (u8_case, u8_eval, u8_check)}
EVAL = {kind: v[1] for kind, v in KINDS.items()}
# deliberately wrong fp32 evaluations: name -> (kind, the check that must catch it)
MUTATIONS = {
    "argsort_unstable": ("argsort", "ids_shuffle"),             # equal values in descending index order
    "mask_gt": ("argsort", "mask"),                             # rank > len_keep
    "gather_column_order": ("gather", "gather"),                # (c, py, px) <-> (py, px, c)
    "gather_gw_from_H": ("gather", "gather"),                   # gw = H / p
    "gather_ids_stride_nsel": ("gather", "gather"),             # ids rows nsel apart
    "ids_stride_nsel": ("tokens", "tok_fwd"),
    "pos_patch_not_shifted": ("tokens", "tok_fwd"),             # pos[patch] for pos[1 + patch]
    "dec_cls_from_row_1": ("decoder", "dec_fwd"),
    "dec_r_le_nkeep": ("decoder", "dec_fwd"),                   # r <= nkeep: the row behind the kept ones
    "dmask_rows_beyond_8_dropped": ("decoder", "dmask"),        # removed rows j >= nkeep + 8
    "dmask_accumulate_ignored": ("decoder", "dmask"),
    "accumulate_ignored": ("dcls", "dcls"),
    "dcls_rows_multiple_of_16": ("dcls", "dcls"),               # B rounded down to a multiple of 16
    "loss_biased_var": ("loss", "loss_dp"),                     # P for P - 1
    "loss_eps_outside_root": ("loss", "loss_dp"),
    "loss_no_2_over_P": ("loss", "loss_dp"),
    "loss_gpp_ignored": ("loss", "loss_dp"),
    "loss_gscale_ignored": ("loss", "loss_dp"),
    "loss_cls_row_nonzero": ("loss", "loss_cls_row"),
    "loss_dpred_not_masked": ("loss", "loss_masked"),
    "loss_gw_from_H": ("loss", "loss_pp"),
    "cast_truncated": ("cast", "cast"),                         # truncation for RNE
    "transpose_edge_swapped": ("transpose", "cast_t"),          # rows <-> cols in the ragged edge guard
    "cast_tail_dropped": ("cast", "cast"),                      # the last n % 4 elements
    "u8_channels_swapped": ("u8", "norm_u8"),
    "u8_div_256": ("u8", "norm_u8"),
}


def make(kind, args):
    return KINDS[kind][0](*args)


def to_device(c, device):
    """the case with `device` noted: the fp32 evaluation moves what it needs, the references stay on the CPU"""
    return dict(c, device=device)


def run_check(c, o, tag="", measure=False, k=None):
    rep = Report(tag or "%s %s %s %s" % (c["kind"], c["family"], dname(c["dtype"]) if c["dtype"] else "-", c["shape"]),
                 measure, k)
    KINDS[c["kind"]][2](c, o, rep)
    return rep


def evaluate(c, mut=None):
    return KINDS[c["kind"]][1](c, mut if mut is not None and MUTATIONS[mut][0] == c["kind"] else None)


# ------------------------------------------------------------------ the case list of the GPU module
DTYPES = (F32, BF)
CAST_N = (0, 1, 3, 4, 5, 1023, 1024, 1025, 4099)
TRANSPOSE_SHAPES = ((1, 1), (1, 33), (33, 1), (31, 32), (32, 32), (33, 65), (45, 70), (64, 96))
TBATCH_MATS = ((64, 64), (65, 63), (4, 8), (1, 130), (130, 1), (68, 132), (3, 5))
ADDCAST_N = (4, 1020, 1024, 1028)
ARGSORT_L, ARGSORT_B = (1, 2, 63, 64, 65, 196, 256, 257, 1024), (1, 3)
GATHER_SHAPES = ((2, 3, 64, 64, 16), (2, 3, 32, 48, 16), (1, 3, 8, 8, 4), (1, 1, 8, 16, 8), (2, 4, 16, 16, 8),
                 (1, 3, 32, 64, 32))
TOKEN_SHAPES = ((1, 1, 4), (2, 3, 8), (3, 4, 128), (2, 5, 252), (2, 3, 1024), (2, 2, 1028))
DCLS_B, DCLS_D = (1, 15, 16, 17, 40), (4, 132)
DECODER_SHAPES = ((1, 1, 0, 4), (1, 1, 1, 4), (2, 16, 4, 128), (3, 9, 9, 8), (2, 9, 0, 8), (2, 12, 9, 8), (2, 20, 1, 1028))
LOSS_SHAPES = ((2, 3, 8, 8, 4), (2, 3, 16, 24, 8), (1, 4, 16, 16, 8), (1, 5, 16, 16, 8), (3, 3, 64, 64, 16),
               (1, 3, 28, 28, 14), (1, 4, 32, 32, 16))
LOSS_FAMILIES = ("gauss", "offset", "const", "integers", "tiny")
# (mask, gpp given, gscale_host): every mask, gpp given and None, both scales
LOSS_COMBOS = (("random", 1, 1.0), ("random", 0, 0.125), ("zeros", 1, 0.125), ("ones", 0, 1.0), ("random", 1, 0.125),
               ("ones", 1, 1.0))
U8_SHAPES = ((1, 1, 4), (2, 2, 2), (3, 30, 28), (1, 7, 12))


def len_keeps(L):
    return tuple(dict.fromkeys((0, 1, L // 4, L)))


def gpu_specs(kind):
    """(group, arguments of the kind's case constructor) of every case tests/test_gpu_mae_kernels.py runs"""
    out = []
    if kind == "cast":
        for dt in DTYPES:
            for n in CAST_N:
                for f in ("gauss", "signed_zero", "specials"):
                    out.append(("%s-n%d" % (dname(dt), n), (f, n, dt)))
    elif kind == "transpose":
        for dt in DTYPES:
            for s in TRANSPOSE_SHAPES:
                for f in ("gauss", "specials"):
                    out.append(("%s-%dx%d" % ((dname(dt),) + s), (f,) + s + (dt,)))
    elif kind == "tbatch":
        out.append(("S7", (TBATCH_MATS,)))
        out.append(("S1", ((TBATCH_MATS[1],),)))
    elif kind == "addcast":
        for n in ADDCAST_N:
            for has_b in (0, 1):
                for want, lp in ((1, None), (0, F32), (0, BF), (1, F32), (1, BF)):
                    for f in ("gauss", "signed_zero"):
                        out.append(("n%d" % n, (f, n, has_b, want, lp)))
    elif kind == "argsort":
        for L in ARGSORT_L:
            for B in ARGSORT_B:
                for keep in len_keeps(L):
                    for f in ("uniform", "ties", "signed_zero"):
                        out.append(("L%d" % L, (f, B, L, keep)))
    elif kind == "gather":
        for dt in DTYPES:
            for s in GATHER_SHAPES:
                for order in (0, 1):
                    for with_ids in (0, 1):
                        out.append(("%s-%dx%dx%dx%d-p%d" % ((dname(dt),) + s),
                                    ("signed_zero" if with_ids else "gauss",) + s + (order, with_ids, dt)))
    elif kind == "tokens":
        for dt in DTYPES:
            for s in TOKEN_SHAPES:
                for with_ids in (0, 1):
                    for f in ("gauss", "signed_zero"):
                        out.append(("%s-%dx%dx%d" % ((dname(dt),) + s), (f,) + s + (dt, with_ids)))
    elif kind == "dcls":
        for B in DCLS_B:
            for D in DCLS_D:
                for acc in (0, 1):
                    for f in ("gauss", "integers"):
                        out.append(("B%d" % B, (f, B, D, acc)))
    elif kind == "decoder":
        for dt in DTYPES:
            for s in DECODER_SHAPES:
                for acc in (0, 1):
                    for f in ("gauss", "integers", "signed_zero"):
                        out.append(("%s-%dx%dx%dx%d" % ((dname(dt),) + s), (f,) + s + (dt, acc)))
    elif kind == "loss":
        for s in LOSS_SHAPES:
            for norm in (0, 1):
                for hc in (0, 1):
                    for i, f in enumerate(LOSS_FAMILIES):
                        for j in range(3):
                            out.append(("%dx%dx%dx%d-p%d-norm%d" % (s + (norm,)),
                                        (f,) + s + (norm, hc) + LOSS_COMBOS[(2 * i + j + hc) % len(LOSS_COMBOS)]))
    elif kind == "u8":
        for s in U8_SHAPES:
            for identity in (0, 1):
                out.append(("%dx%dx%d" % s, s + (identity,)))
    return out


def groups(specs):
    return list(dict.fromkeys(s[0] for s in specs))


def measure_k_ref(device, log=print):
    """worst error / (2^-24 mag) per bounded check of the fp32 torch evaluation over the GPU module's case list"""
    worst = {}
    for kind in ("dcls", "decoder", "loss", "u8"):
        for grp, a in gpu_specs(kind):
            c = to_device(make(kind, a), device)
            rep = run_check(c, evaluate(c), measure=True)
            for n, v in rep.worst.items():
                if n in BOUNDED and v > worst.get(n, 0.0):
                    worst[n] = v
                    log("k_ref %s = %.3f at %s %s %s" % (n, v, kind, grp, a[0]))
    return worst
