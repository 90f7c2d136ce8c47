"""fp64 reference of softmax attention on the packed qkv[B, N, 3, H, hd] layout and the per-element checks that pin
every variant behind ssl4gie_attn_fwd / ssl4gie_attn_bwd (csrc/attention.hip) to it
(tests/test_gpu_attention_kernels.py; proof that the checks bite: tests/test_attn_checks_cpu.py).

Reference.  scale = hd^-1/2, S = scale Q K^T, per (batch, head):
  `ref_forward`:   lse = log sum_j exp S_ij,  P = exp(S - lse),  O = P V
  `ref_backward`:  evaluated from exactly what the kernel is handed (the convention of bn_checks) — the stored O
                   and the stored fp32 lse — so that a forward error is charged to the forward checks and to nothing
                   else:   P = exp(S - lse_given),  delta_i = sum_d dO_id O_given_id,  dP = dO V^T,
                   dS = P (dP - delta),  dV = P^T dO,  dQ = scale dS K,  dK = scale dS^T Q.

Bounds, per element, never a global max-norm:

    |got - ref| <= u (|ref| + c mag_u) + k 2^-24 mag_24          u = 2^-8 on the bf16 path, 0 on the fp32 path
(plus 2^-100 absolute, the underflow floor of fp32: see UNDERFLOW)

Derivation of c.  The interface fixes three roundings to bf16 and no more: the operands are bf16 (shared with the
reference), the output is rounded once (u |ref|), and each probability — in the backward each dS — is rounded once
before its second product, because it is the bf16 operand of the next MFMA.  With p~_j = p_j (1 + e_j), |e_j| <= u:
    | sum_j p~_j v_jd - sum_j p_j v_jd | <= u sum_j p_j |v_jd|
and all accumulation is fp32 (the k term).  Hence c = 1 with
    O    mag_u = sum_j p_ij |v_jd|                  dQ   mag_u = scale sum_j |dS_ij| |K_jd|
    dV   mag_u = sum_i p_ij |dO_id|                 dK   mag_u = scale sum_i |dS_ij| |Q_id|
Where the normaliser of O is the sum of the ROUNDED probabilities, sum_j p~_j = (sum_j p_j)(1 + e), |e| <= u, O
carries another u |O| <= u mag_u: c = 2 for O, and lse = m + log sum p~ is off by |log(1 + e)| <= u in absolute
terms (`lse_u`).  Under the fp32 sum of the unrounded probabilities both are 0.  Which convention a kernel family
follows is read from its source (NORMALISER below); the checks take it from `family_of`.
When every probability is exactly representable (families `uniform` and `onehot`: p~ = p = 1 or 0 before the
division) no rounding of P happens in the forward: the c term of O and the lse_u term are dropped under EITHER
convention (`exact_p`), and lse is pinned at the 2^-24 level — a dropped, duplicated or leaked key is a 1 / N error
there.

mag_24: the fp64 sum of the absolute values of every term that is added,
    O    sum_j p_ij |v_jd|          dV   sum_i p_ij |dO_id|
    dQ   scale sum_j p_ij a_ij |K_jd|,   dK   scale sum_i p_ij a_ij |Q_id|,
         a_ij = sum_d |dO_id V_jd| + sum_d |dO_id O_id|       (|dP - delta| with its terms taken absolutely)
    lse  sum_j p_ij scale sum_d |q_id k_jd| + |lse| + 1

k.  Procedure (that of bn_checks): the same formulae in plain fp32 torch with the roundings the interface implies
(`emu_eval`: P and dS rounded to bf16 before their second products, fp32 accumulation, bf16 outputs, either
normaliser convention; no rounding at all for the fp32 path) — neither the kernels nor the engine — run through
these checks over the case list of the GPU module (`measure_k_ref`); the worst (error beyond the u terms) /
(2^-24 mag_24) per check is k_ref, and k = max(16, 4 k_ref) rounded up to a power of two: the kernels' dependent-add
chains, the hardware exp2 / log and the exp2-domain arithmetic (S c - m c, c = scale log2 e) differ from torch's at
the 2^-24 level only.  k is kept per path (bf16 | fp32) and check: on the fp32 path there are no u terms, every error
lands on k, and the rounding of the exponent S - lse — an absolute error of 2^-24 |S| in the exponent, a relative one
in every probability, |S| up to ~300 in `gauss` at scale 3 and hd 80 — is not a term of mag_24: it is what k_ref
measures there.  Measured k_ref (K_REF below) -> k (K below); the larger of torch on the CPU (every case up to
N = 1024) and torch on the MI355X (the whole list):

    check      k_ref (CPU)   k_ref (MI355X)      k
    bf16.o          0.000            0.000      16
    bf16.lse        1.634            2.333      16
    bf16.dq         0.659            0.585      16
    bf16.dk         0.527            0.287      16
    bf16.dv         0.000            0.000      16
    fp32.o        201.800          321.700    2048
    fp32.lse        3.130            3.031      16
    fp32.dq        66.870           40.940     512
    fp32.dk        49.650           51.900     256
    fp32.dv       351.000          252.800    2048

On the bf16 path the emulation's error is inside the u terms wherever they exist (bf16.o, bf16.dv: no excess at
all; dq, dk: below one 2^-24 mag_24): the worst |error| / (u (|ref| + c mag_u)) it reached over the `gauss` cases is
recorded in U_REF — o 0.86, dq 0.94, dk 0.94, dv 0.95 of the derived bound, lse 0.43 of its u.  The derived c holds
for the reference itself, with little room to spare; the 2^-24 term decides where the u terms vanish (fp32 path,
`uniform`, `onehot`).
The kernels themselves, over the whole GPU module (the figures the k above leave room for): bf16.o 0.0, bf16.lse 2.56,
bf16.dq 0.80, bf16.dk 0.15, bf16.dv 0.0, fp32.o 350, fp32.lse 2.97, fp32.dq 40.8, fp32.dk 55.5, fp32.dv 280; share
of the u terms: o 0.87, lse 0.40, dq 0.93, dk 0.94, dv 0.94.
"""
import math

import torch

EPS32 = 2.0 ** -24
U_BF16 = 2.0 ** -8
F64, F32, BF = torch.float64, torch.float32, torch.bfloat16
CHECKS = ("o", "lse", "dq", "dk", "dv")
# absolute floor of every bound: fp32 has no values below 2^-126 (2^-149 with denormals, which the hardware exp2
# flushes), fp64 does — a probability of e^-181 is 0 in the kernels and 1e-79 in the reference.  What is lost is at
# most N max|operand|^2 2^-126 < 2^-100 for every case here (N <= 4096, operands <= 32).
UNDERFLOW = 2.0 ** -100

# kernel family -> (normaliser of O / argument of the log in lse, the source it rests on: csrc/attention.hip)
NORMALISER = {
    "whole32": ("rounded", "attn_fwd_bf16_kernel, MSUM = HD == 32: `osum = MFMA16(ones, pf, osum)` — \"That sum is the one "
                           "of the bf16-rounded probabilities, i.e. of exactly the values O^T = V^T P^T is accumulated from\""),
    "whole64": ("fp32", "attn_fwd_bf16_kernel, !MSUM: `sum2 += a; sum2 += bq;` on the fp32 exp2 results, before pack8 "
                        "— \"hd 64 ... keeps the packed fp32 adds\""),
    "stream": ("fp32", "attn_long_fwd_kernel, both hd: `sum += pp;` on the fp32 exp2 result, `lsum = lsum * alpha + sum`; "
                       "pack8 rounds afterwards"),
    "fp32": ("fp32", "softmax_rows_kernel: fp32 throughout, nothing is rounded"),
}


def family_of(dtype, N, hd):
    """the kernel family ssl4gie_attn_fwd dispatches (dtype, N, hd) to, at the default environment"""
    if dtype != BF:
        return "fp32"
    assert hd in (32, 64)
    return "stream" if N > 256 else "whole%d" % hd


def nkt_of(N):
    """16-key tiles of the whole-head kernels' bucket: 16 (NKT - 2) < N <= 16 NKT"""
    return 2 * max(1, (N + 31) >> 5)


# worst (error beyond the u terms) / (2^-24 mag_24) of `emu_eval` over the GPU module's case list (measure_k_ref)
# keys: "<path>.<check>", path = bf16 | fp32 (see the docstring)
K_REF_CPU = {"bf16.o": 0.0, "bf16.lse": 1.634, "bf16.dq": 0.659, "bf16.dk": 0.527, "bf16.dv": 0.0,
             "fp32.o": 201.8, "fp32.lse": 3.130, "fp32.dq": 66.87, "fp32.dk": 49.65, "fp32.dv": 351.0}      # torch, CPU
K_REF_GPU = {"bf16.o": 0.0, "bf16.lse": 2.333, "bf16.dq": 0.585, "bf16.dk": 0.287, "bf16.dv": 0.0,
             "fp32.o": 321.7, "fp32.lse": 3.031, "fp32.dq": 40.94, "fp32.dk": 51.90, "fp32.dv": 252.8}      # torch, MI355X
K_REF = {n: max(K_REF_CPU[n], K_REF_GPU[n]) for n in K_REF_CPU}
# worst |error| / (u (|ref| + c mag_u)) of the bf16 emulation over the same list (1 = the derived bound)
U_REF = {"o": 0.862, "lse": 0.426, "dq": 0.938, "dk": 0.944, "dv": 0.953}


def k_from(k_ref):
    return max(16, 2 ** math.ceil(math.log2(max(4.0 * k_ref, 1.0))))


K = {name: k_from(v) for name, v in K_REF.items()}


class Report:
    """worst (error beyond the u terms) / (2^-24 mag_24) per check, the worst share of the u terms used, and the
    checks that exceeded their k"""

    def __init__(self, k=None, tag="", measure=False):
        self.k = K if k is None else k
        self.tag = tag
        self.measure = measure      # record the ratios, fail none (k_ref)
        self.path = "bf16"          # set by check_forward / check_backward from the case's dtype
        self.share = False          # record the share of the u terms used (gauss cases)
        self.worst = {}
        self.worst_u = {}
        self.failed = []

    def ratio(self, name, got, ref, mag_u, mag_24, u=0.0, c=1.0, abs_u=0.0):
        got = got.to(F64)
        diff = (got - ref).abs()
        ub = u * (ref.abs() + c * mag_u) + abs_u if (u or abs_u) else None
        err = ((diff if ub is None else diff - ub) - UNDERFLOW).clamp_min(0)
        r = err / (EPS32 * mag_24)
        r = torch.where(err == 0, torch.zeros_like(r), r)           # 0 / 0: an exact value
        r = torch.nan_to_num(r, nan=math.inf, posinf=math.inf).reshape(-1)
        m, i = r.max(0)
        if ub is not None and self.share:
            s = (diff - 16 * EPS32 * mag_24 - UNDERFLOW).clamp_min(0)       # what the smallest k term does not cover
            s = torch.where(s == 0, torch.zeros_like(s), s / ub)
            self.worst_u[name] = max(self.worst_u.get(name, 0.0), float(torch.nan_to_num(s, nan=math.inf).max()))
        self.note(name, float(m), "at flat index %d of shape %s (got %r, ref %r)"
                  % (int(i), tuple(got.shape), float(got.reshape(-1)[i]), float(ref.reshape(-1)[i])))

    def note(self, name, value, where=""):
        key = self.path + "." + name
        self.worst[key] = max(self.worst.get(key, 0.0), value)
        if not value <= self.k[key] and not self.measure:
            self.failed.append("%s %s: error beyond the u terms = %.4g x 2^-24 mag > k = %g %s"
                               % (self.tag, name, value, self.k[key], where))

    def fail(self, name, msg):
        if self.measure:
            return
        self.worst[self.path + "." + name] = math.inf
        self.failed.append("%s %s: %s" % (self.tag, name, msg))

    def names(self):
        return sorted({f.split(":")[0].split()[-1] for f in self.failed})

    def assert_ok(self):
        assert not self.failed, "\n".join(self.failed[:40])


# ------------------------------------------------------------------ fp64 reference
def heads(t, B, N, H, hd):
    """[B, N, H hd] -> [B, H, N, hd]"""
    return t.reshape(B, N, H, hd).permute(0, 2, 1, 3)


def split_qkv(qkv, B, N, H, hd, dt):
    q, k, v = qkv.reshape(B, N, 3, H, hd).to(dt).permute(2, 0, 3, 1, 4).unbind(0)
    return q, k, v      # [B, H, N, hd] views


def _row_block(B, N, H):
    return max(1, min(N, (1 << 24) // max(1, B * H * N)))    # <= 128 MiB of fp64 per N x N temporary


def ref_forward(qkv, B, N, H, hd):
    """fp64 O [B, N, H hd], lse [B, H, N] and the magnitudes of their bounds (mag_o = sum_j p |v|: both mag_u and
    mag_24 of O; mag_lse), in query row blocks"""
    q, k, v = split_qkv(qkv, B, N, H, hd, F64)
    scale = hd ** -0.5
    O = torch.empty(B, H, N, hd, dtype=F64, device=qkv.device)
    mag_o, lse, mag_lse = torch.empty_like(O), O.new_empty(B, H, N), O.new_empty(B, H, N)
    kt, ka, va = k.transpose(-1, -2), k.abs().transpose(-1, -2), v.abs()
    rb = _row_block(B, N, H)
    for r0 in range(0, N, rb):
        r = slice(r0, min(N, r0 + rb))
        s = (q[:, :, r] @ kt) * scale
        l = torch.logsumexp(s, -1)
        p = (s - l.unsqueeze(-1)).exp()
        O[:, :, r], mag_o[:, :, r], lse[:, :, r] = p @ v, p @ va, l
        mag_lse[:, :, r] = (p * ((q[:, :, r].abs() @ ka) * scale)).sum(-1) + l.abs() + 1.0
    back = lambda t: t.permute(0, 2, 1, 3).reshape(B, N, H * hd)
    return {"o": back(O), "mag_o": back(mag_o), "lse": lse, "mag_lse": mag_lse}


def ref_backward(qkv, o_given, do, lse_given, B, N, H, hd):
    """fp64 backward from the handed (O [B, N, H hd], lse [B, H, N]) -> dict of dq, dk, dv [B, H, N, hd] with their
    mag_u (`u_*`) and mag_24 (`m_*`)"""
    q, k, v = split_qkv(qkv, B, N, H, hd, F64)
    scale = hd ** -0.5
    dO, Og = heads(do.to(F64), B, N, H, hd), heads(o_given.to(F64), B, N, H, hd)
    lse = lse_given.to(F64)
    z = lambda: torch.zeros(B, H, N, hd, dtype=F64, device=qkv.device)
    o = {n: z() for n in ("dq", "dk", "dv", "u_dq", "u_dk", "u_dv", "m_dq", "m_dk")}
    kt, vt = k.transpose(-1, -2), v.transpose(-1, -2)
    rb = _row_block(B, N, H)
    for r0 in range(0, N, rb):
        r = slice(r0, min(N, r0 + rb))
        qr, dOr, Or = q[:, :, r], dO[:, :, r], Og[:, :, r]
        p = ((qr @ kt) * scale - lse[:, :, r].unsqueeze(-1)).exp()
        delta = (dOr * Or).sum(-1, keepdim=True)
        ds = p * (dOr @ vt - delta)
        pa = p * (dOr.abs() @ vt.abs() + (dOr * Or).abs().sum(-1, keepdim=True))
        pt, dst = p.transpose(-1, -2), ds.transpose(-1, -2)
        o["dv"] += pt @ dOr
        o["u_dv"] += pt @ dOr.abs()
        o["dq"][:, :, r] = scale * (ds @ k)
        o["u_dq"][:, :, r] = scale * (ds.abs() @ k.abs())
        o["m_dq"][:, :, r] = scale * (pa @ k.abs())
        o["dk"] += scale * (dst @ qr)
        o["u_dk"] += scale * (dst.abs() @ qr.abs())
        o["m_dk"] += scale * (pa.transpose(-1, -2) @ qr.abs())
    o["m_dv"] = o["u_dv"]
    return o


def check_forward(rep, c, o, lse, tag="", fw=None):
    """O [B, N, H hd] and lse [B, H, N] of case `c` against fp64, under the convention of the case's kernel family"""
    B, N, H, hd = c["B"], c["N"], c["H"], c["hd"]
    fw = fw or ref_forward(c["qkv"], B, N, H, hd)
    u = U_BF16 if c["dtype"] == BF else 0.0
    rep.path, rep.share = ("bf16" if u else "fp32"), c["family"] == "gauss"
    rounded = u > 0 and NORMALISER[c["kernel"]][0] == "rounded"
    exact = c["exact_p"]
    rep.ratio("o", o, fw["o"], fw["mag_o"], fw["mag_o"], u, 0.0 if exact else (2.0 if rounded else 1.0))
    rep.ratio("lse", lse, fw["lse"], fw["mag_lse"], fw["mag_lse"], 0.0, 0.0, U_BF16 if rounded and not exact else 0.0)
    if c["family"] == "onehot":
        sel = c["qkv"].reshape(B, N, 3, H, hd)[:, :, 2].to(F64).permute(0, 2, 1, 3)     # V [B, H, N, hd]
        sel = torch.gather(sel, 2, c["perm"].view(1, 1, N, 1).expand(B, H, N, hd))
        if not torch.equal(heads(o.to(F64), B, N, H, hd), sel):
            rep.fail("o", "onehot: O is not the selected V row at %d elements"
                     % int((heads(o.to(F64), B, N, H, hd) != sel).sum()))
    return fw


def check_backward(rep, c, o_given, lse_given, dqkv, tag=""):
    """dqkv [B, N, 3, H, hd] against the fp64 backward from the handed (O, lse)"""
    B, N, H, hd = c["B"], c["N"], c["H"], c["hd"]
    bw = ref_backward(c["qkv"], o_given, c["do"], lse_given, B, N, H, hd)
    u = U_BF16 if c["dtype"] == BF else 0.0
    rep.path, rep.share = ("bf16" if u else "fp32"), c["family"] == "gauss"
    got = dqkv.reshape(B, N, 3, H, hd).permute(2, 0, 3, 1, 4)
    for i, n in enumerate(("dq", "dk", "dv")):
        rep.ratio(n, got[i], bw[n], bw["u_" + n], bw["m_" + n], u, 1.0)
    if c["family"] == "onehot":
        dO = heads(c["do"].to(F64), B, N, H, hd)
        inv = torch.empty_like(c["perm"])
        inv[c["perm"]] = torch.arange(N, device=inv.device)
        want = torch.gather(dO, 2, inv.view(1, 1, N, 1).expand(B, H, N, hd))    # dV_j = dO of the query that chose j
        if not torch.equal(got[2].to(F64), want):
            rep.fail("dv", "onehot: dV is not the permuted dO at %d elements" % int((got[2].to(F64) != want).sum()))
    return bw


def check_all(c, o, k=None, tag="", measure=False):
    """every check of this module on the outputs `o` = (O, lse, dqkv) of case `c`; the backward is judged from the
    (O, lse) in `o`"""
    rep = Report(k, tag or c["tag"], measure)
    check_forward(rep, c, o[0], o[1])
    if o[2] is not None:
        check_backward(rep, c, o[0], o[1], o[2])
    return rep


# ------------------------------------------------------------------ cases (generated on the CPU from fixed seeds)
GAUSS_VARIANTS = ((0.5, False), (1.5, False), (3.0, False), (1.5, True))     # (scale, per-head mean offset on q, k)
UNIFORM_S0 = (0, -1, 1)         # the common score: 0, about -32, about +32


def uniform_consts(hd, sign):
    """(a, b): q = a, k = b everywhere, s0 = hd^1/2 a b ~ 32 sign; a a multiple of 1/4 (exact in bf16)"""
    if sign == 0:
        return 1.0, 0.0
    return round(32.0 / (2.0 * math.sqrt(hd)) * 4) / 4, 2.0 * sign


def onehot_code(N, hd):
    """[N, hd]: row j spells hd / 2 bits — the low byte of j, then the bytes ((j >> 8) + 37 j + 11) mod 256, ... (which
    tell apart two j with the same low byte) — one pair of columns per bit, (g, 0) or (0, g), g = 32: rows j != j'
    differ in at least one bit, so q_i . k_j <= q_i . k_i - g^2 and every other probability is below
    exp(-g^2 hd^-1/2) <= e^-128: exactly 0 in fp32, with or without denormals"""
    assert N <= 65536 and hd >= 32
    j = torch.arange(N)
    code = torch.zeros(N, hd)
    for t in range(hd // 2):
        b = (t // 8) % 4
        byte = (j * (1, 37, 101, 201)[b] + (0, 11, 67, 5)[b] + (j >> 8 if b else 0)) % 256
        bit = (byte >> (t % 8)) & 1
        code[j, 2 * t + bit] = 32.0
    return code


def make_case(family, B, N, H, hd, dtype, seed=0, scale=1.5, offset=False, s0=0):
    """-> dict: qkv [B, N, 3, H, hd], do [B, N, H hd] (already rounded to `dtype`, on the CPU) + what the checks need"""
    g = torch.Generator("cpu").manual_seed(1000003 * seed + 7919 * N + 31 * hd + H)
    rn = lambda *s: torch.randn(*s, generator=g)
    ri = lambda *s: torch.randint(-4, 5, s, generator=g).float()
    c = {"family": family, "B": B, "N": N, "H": H, "hd": hd, "dtype": dtype, "kernel": family_of(dtype, N, hd),
         "exact_p": family != "gauss", "perm": None}
    if family == "gauss":
        qkv = rn(B, N, 3, H, hd) * scale
        if offset:      # a trained network's q and k have a per-head mean: it shifts every score
            qkv[:, :, :2] += 0.5 * scale * rn(1, 1, 2, H, hd)
        do = rn(B, N, H * hd)
        c["tag"] = "gauss(%g%s)" % (scale, "+mean" if offset else "")
    elif family == "uniform":
        a, b = uniform_consts(hd, s0)
        qkv = torch.empty(B, N, 3, H, hd)
        qkv[:, :, 0], qkv[:, :, 1], qkv[:, :, 2] = a, b, ri(B, N, H, hd)
        do = ri(B, N, H * hd)
        c["tag"] = "uniform(s0=%+.3g)" % (math.sqrt(hd) * a * b)
    else:
        assert family == "onehot"
        code = onehot_code(N, hd)
        perm = torch.randperm(N, generator=g)
        qkv = torch.empty(B, N, 3, H, hd)
        qkv[:, :, 0] = code[perm].view(1, N, 1, hd)           # query i matches key perm[i]
        qkv[:, :, 1] = code.view(1, N, 1, hd)
        v = ri(B, N, H, hd)
        v[:, :, :, :8] = ((torch.arange(N).view(N, 1) >> torch.arange(8)) & 1).float().view(1, N, 1, 8)
        qkv[:, :, 2] = v
        do = ri(B, N, H * hd)
        c["perm"] = perm
        c["tag"] = "onehot"
    c["qkv"], c["do"] = qkv.to(dtype).contiguous(), do.to(dtype).contiguous()
    c["tag"] += " B%d N%d H%d hd%d %s" % (B, N, H, hd, "bf16" if dtype == BF else "fp32")
    return c


def to_device(c, device):
    return {k: v.to(device) if torch.is_tensor(v) else v for k, v in c.items()}


# ------------------------------------------------------------------ the same formulae in plain fp32 torch
MUTATIONS = ("drop_last_key", "dup_key", "pad_leak", "swap_v", "wrong_scale", "lse_no_max", "lse_base2", "row_dup",
             "last_strip", "head_swap", "no_delta", "dk_no_scale", "dq_dk_exchanged", "lse_neighbour", "dv_wrong_head")


def emu_eval(c, normaliser=None, mut=None, backward=True):
    """forward + backward of case `c` in fp32 torch with the roundings the interface implies (bf16 cases: P and dS
    rounded before their second products, outputs rounded; fp32 cases: none).  `normaliser`: "rounded" / "fp32"
    (default: the case's kernel family's).  `mut`: one of MUTATIONS — a deliberately wrong variant
    (tests/test_attn_checks_cpu.py).  -> (O [B, N, H hd], lse [B, H, N] fp32, dqkv [B, N, 3, H, hd] or None)"""
    B, N, H, hd, dt = c["B"], c["N"], c["H"], c["hd"], c["dtype"]
    normaliser = normaliser or NORMALISER[c["kernel"]][0]
    rnd = (lambda t: t.to(BF).to(F32)) if dt == BF else (lambda t: t)
    q, k, v = split_qkv(c["qkv"], B, N, H, hd, F32)
    dO = heads(c["do"].to(F32), B, N, H, hd)
    scale = ((32 if hd == 64 else 64) if mut == "wrong_scale" else hd) ** -0.5     # the other head size's
    kf, vf = k, v               # the keys the forward sees
    if mut == "drop_last_key" and N > 1:
        kf, vf = k[:, :, :-1], v[:, :, :-1]
    elif mut == "dup_key":
        kf, vf = torch.cat([k, k[:, :, :1]], 2), torch.cat([v, v[:, :, :1]], 2)
    elif mut == "pad_leak":     # one zero-padded key row joins the softmax
        kf, vf = torch.cat([k, torch.zeros_like(k[:, :, :1])], 2), torch.cat([v, torch.zeros_like(v[:, :, :1])], 2)
    elif mut == "swap_v" and N > 1:
        vf = v.clone()
        vf[:, :, 0], vf[:, :, 1] = v[:, :, 1], v[:, :, 0]
    s = (q @ kf.transpose(-1, -2)) * scale
    m = s.max(-1, keepdim=True).values
    e = (s - m).exp()
    pt = rnd(e)
    tot = (pt if normaliser == "rounded" else e).sum(-1, keepdim=True)
    O = (pt @ vf) / tot
    lse = (tot.log() if mut == "lse_no_max" else m + tot.log()).squeeze(-1)
    if mut == "lse_base2":
        lse = lse * 1.4426950408889634
    back = lambda t: t.permute(0, 2, 1, 3).reshape(B, N, -1)
    if mut == "row_dup" and N > 1:
        O[:, :, N - 2], lse[:, :, N - 2] = O[:, :, N - 1], lse[:, :, N - 1]
    if mut == "head_swap":
        O = O[:, [h ^ 1 if (h ^ 1) < H else h for h in range(H)]]
    O = back(O).to(dt)
    if mut == "last_strip":
        O.view(B, N, H, hd)[..., -8:] = 0
    if not backward:
        return O, lse, None
    # backward, from the stored (O, lse) as the kernels do; the mutated lse conventions are undone first so that
    # each wrong variant is wrong in one place only
    l = lse
    if mut == "lse_base2":
        l = lse / 1.4426950408889634
    elif mut == "lse_no_max":
        l = lse + m.squeeze(-1)
    if mut == "lse_neighbour":
        l = l.roll(1, -1)
    scale = hd ** -0.5
    p = ((q @ k.transpose(-1, -2)) * scale - l.unsqueeze(-1)).exp()
    dp = dO @ v.transpose(-1, -2)
    delta = (dO * heads(O.to(F32), B, N, H, hd)).sum(-1, keepdim=True)
    ds = rnd(p * (dp if mut == "no_delta" else dp - delta))
    pv = rnd(p)
    if mut == "dv_wrong_head":
        pv = pv[:, [h ^ 1 if (h ^ 1) < H else h for h in range(H)]]
    dv = pv.transpose(-1, -2) @ dO
    dq = scale * (ds @ k)
    dk = (1.0 if mut == "dk_no_scale" else scale) * (ds.transpose(-1, -2) @ q)
    if mut == "dq_dk_exchanged":
        dq, dk = dk, dq
    dqkv = torch.stack([dq, dk, dv]).permute(1, 3, 0, 2, 4).contiguous().to(dt)      # [B, N, 3, H, hd]
    if mut == "last_strip":
        dqkv[..., -8:] = 0
    return O, lse, dqkv


# ------------------------------------------------------------------ the case list of the GPU module
def whole_head_edges():
    """every N at which a whole-head bucket changes behaviour: for NKT = 2 ... 16, the bucket's first N, the last
    half-tail N, the first N with one key in the last tile, and the full bucket; plus N = 1"""
    ns = {1}
    for nkt in range(2, 17, 2):
        ns |= {16 * (nkt - 2) + 1, 16 * (nkt - 1), 16 * (nkt - 1) + 1, 16 * nkt}
    return sorted(ns)


STREAM_N = (257, 300, 383, 384, 385, 512, 1000, 1024, 4096)
FP32_N, FP32_HD = (1, 17, 50, 197, 384), (8, 32, 48, 64, 80)
ONE_PER_BUCKET = (1, 20, 50, 90, 128, 150, 177, 197, 256)        # NKT 2, 2, 4, 6, 8, 10, 12, 14, 16
PRODUCTION = ((64, 50, 12, 64), (64, 197, 16, 32), (64, 197, 12, 64), (64, 197, 12, 32), (2, 1024, 12, 64))


def stream_bh(N):
    return (1, 2) if N >= 4096 else (2, 3)


def case_list(max_n=None):
    """(family, B, N, H, hd, dtype, kwargs) of every reference-checked case of the GPU module except the dense
    1 ... 256 sweep (represented by one N per bucket) and the production batches"""
    out = []
    for hd in (32, 64):
        for N in whole_head_edges():
            for sc, off in GAUSS_VARIANTS:
                out.append(("gauss", 2, N, 3, hd, BF, {"scale": sc, "offset": off}))
        for N in ONE_PER_BUCKET:
            for s0 in UNIFORM_S0:
                out.append(("uniform", 1, N, 2, hd, BF, {"s0": s0}))
            out.append(("onehot", 1, N, 2, hd, BF, {}))
        for N in STREAM_N:
            B, H = stream_bh(N)
            for sc, off in GAUSS_VARIANTS:
                out.append(("gauss", B, N, H, hd, BF, {"scale": sc, "offset": off}))
            for s0 in UNIFORM_S0:
                out.append(("uniform", B, N, H, hd, BF, {"s0": s0}))
            if N <= 1024:
                out.append(("onehot", B, N, H, hd, BF, {}))
    for hd in FP32_HD:
        for N in FP32_N:
            for sc, off in GAUSS_VARIANTS:
                out.append(("gauss", 2, N, 3, hd, F32, {"scale": sc, "offset": off}))
            for s0 in UNIFORM_S0:
                out.append(("uniform", 2, N, 3, hd, F32, {"s0": s0}))
    return [x for x in out if max_n is None or x[2] <= max_n]


def measure_k_ref(device, cases=None, log=print):
    """worst ratios of emu_eval over `cases` (default: case_list()), both normaliser conventions on the bf16 path
    -> (k_ref per check, worst share of the u terms per check)"""
    worst, worst_u = {}, {}
    for i, (fam, B, N, H, hd, dtype, kw) in enumerate(cases or case_list()):
        c = to_device(make_case(fam, B, N, H, hd, dtype, seed=i, **kw), device)
        for norm in (("rounded", "fp32") if dtype == BF else ("fp32",)):
            c["kernel"] = {"rounded": "whole32", "fp32": "whole64" if dtype == BF else "fp32"}[norm]
            rep = check_all(c, emu_eval(c, norm), measure=True)
            for n, v in rep.worst.items():
                if v > worst.get(n, 0.0):
                    worst[n] = v
                    log("k_ref %s = %.3f at %s (%s)" % (n, v, c["tag"], norm))
            for n, v in rep.worst_u.items():
                if v > worst_u.get(n, 0.0):
                    worst_u[n] = v
                    log("u share %s = %.3f at %s (%s)" % (n, v, c["tag"], norm))
        del c
    return worst, worst_u
