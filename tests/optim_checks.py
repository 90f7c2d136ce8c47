"""fp64 references of the arena AdamW and LARS steps and the per-element checks that pin `adamw_arena_kernel` and the
three LARS kernels of optim_ops.hip to them (tests/test_gpu_optim_kernels.py; proof that the checks bite:
tests/test_optim_checks_cpu.py).

References: plain torch on the CPU in float64, starting from exactly what the kernel is handed.  p, g, m, v, mu are
the fp32 values converted to double; beta1, beta2, eps, lr, wd, momentum, trust and ctl[1] are first rounded to fp32
and then used as doubles, as the ABI carries them (the convention of `ema` in map_checks).
  AdamW (`adamw_ref`), t = `step` when host-counted and *applied + 1 when device-counted, c = ctl[1] or 1:
    g' = c g;  m' = b1 m + (1 - b1) g';  v' = b2 v + (1 - b2) g'^2;  bc1 = 1 - b1^t, bc2 = 1 - b2^t
    den = sqrt(v') / sqrt(bc2) + eps;  upd = (lr / bc1) m' / den;  p' = p (1 - lr wd) - upd
    lp' = bf16(p_out), from the kernel's OWN fp32 output, round to nearest even
  LARS (`lars_ref`), per segment:
    matrix (seg_mat != 0): d = g + wd p; q = trust |p| / |d| if both norms > 0, else 1; dp = d q
    vector:                dp = g (no weight decay, no trust ratio)
    mu' = momentum mu + dp;  p' = p - lr mu'

Two kinds of check, per output element, never a global norm.
  Bounded: |got - ref| <= slack + k 2^-24 mag, mag = the fp64 sum of the ABSOLUTE values of the terms the kernel adds,
  the propagated terms written out:
    adamw_m   |b1 m| + |(1 - b1) g'|
    adamw_v   v'                                      (both terms are non-negative)
    adamw_p   |p| + (lr / bc1) mag_m / den            (the second term carries the cancellation of m' into the update)
    lars_mu   |momentum mu| + (|g| + |wd p|) q        (vector: |momentum mu| + |g|)
    lars_p    |p| + lr mag_mu
  slack (adamw_p only) = |upd| 2^-23 (b1^t / bc1 + 1/2 b2^t / bc2), DERIVED, not measured: the kernel and its host
  wrapper form 1 - powf(b, t) in fp32; one ulp of powf (at most 2^-23 b^t) is a relative error of 2^-23 b^t / (1 - b^t)
  of the bias correction, the square root halves the b2 share.  It is charged outside k, as map_checks charges the
  bilinear coordinate.  Without it the fp32 restatement reaches 56 x 2^-24 mag on adamw_p (b2 = 0.999, t = 2): a k of
  16 would fail correct code and a k that passes would pin nothing.
  Bit for bit (`Report.bits`: the int views, so that NaN patterns and the sign of zero count):
    lp          equals p_out.to(bfloat16) wherever an update was applied
    untouched   p, m, v, mu and lp of every skipped segment (seg_lr < 0; padding included), everything outside
                [lo, hi) (LARS: outside the sub-range it was handed) and the 256-element bands around every buffer are
                bit-unchanged.  The case builders poison g over skipped segments with NaN: their gradient slice "may
                hold stale values and is not read"
    g           bit-unchanged everywhere, also with ctl[1] != 1
    pad_zero    the zero tail of an active segment stays +0 in p, m, v (mu); every layout has such tails
    applied     device-counted with advance: *applied becomes t
  LARS takes q = 1 and stays finite in a matrix segment whose p is all zero and in one whose g + wd p is all zero
  (g = 0 under a table entry wd = 0): a NaN fails lars_mu / lars_p (`Report.ratio` turns it into inf).
Every case of the list goes through every check of its optimizer; no family is left out.

k.  Procedure (as in bn_checks / attn_checks / ln_checks / map_checks): evaluate the same formulae in plain fp32
torch (`adamw_eval`, `lars_eval`: neither the kernels nor optim.py; AdamW in the kernel's order of operations, the two
LARS norms summed in the kernel's order: 32 parts x 256 threads x 4 lanes in strided trips of 32 x 1024, a running sum
per thread, then the wave tree, the four waves in sequence and the 32 parts in sequence), run it through these checks
over the case list of the GPU module (`measure_k_ref`), record the worst error / (2^-24 mag) per check as k_ref — the
larger of torch on the CPU and torch on the MI355X — and set k = max(16, 4 k_ref) rounded up to a power of two.  No k
comes from the kernels' own ratios.  The kernels' column is what the last test of tests/test_gpu_optim_kernels.py
printed on an MI355X.

    check      k_ref CPU  k_ref MI355X  k     kernels' worst ratio
    adamw_m        2.14         2.14    16     2.24
    adamw_v        3.47         3.47    16     3.58
    adamw_p        3.71         3.71    16     3.36
    lars_mu        4.58         4.58    32     4.79
    lars_p         2.62         2.62    16     1.71
adamw_p stays inside the derived slack on the device-counted path too (device powf).  lars_mu: the 4.58 is a
64-element matrix segment of `many` at momentum 0, where mu' is d q alone and carries the rounding of d, of both norms,
of their square roots, of the product and the quotient in q and of d q; over the other layouts it stays below 3.9.

The betas (not gated, `beta_rounding_deviation`).  The reference uses the betas as rounded to fp32; torch.optim.AdamW
uses the Python doubles: 1 - 0.999f differs from 0.001 by 1.3e-5 relative, 1 - 0.9f from 0.1 by 2.4e-7.  This is a
property of the ABI, not a kernel error, and the checks do not see it.  Worst relative deviation of upd, fp32-rounded
betas against double betas, both in fp64 over t steps from m = v = 0 on the same gaussian gradients, over the updates
of at least 1 % of the largest (at t = 1 the betas cancel out of m' / bc1 and v' / bc2; from there the deviation
grows with the history the moments hold, and an m' that is itself the rest of a cancellation magnifies it):
    (b1, b2)        t = 1      t = 10     t = 1000
    (0.9, 0.95)     < 1e-15    4.0e-6     1.1e-5
    (0.9, 0.999)    < 1e-15    5.1e-6     8.2e-6

Input families (generated on the CPU from fixed seeds; every value and every square well inside the normal fp32
range, v >= 0):
    gauss     p, g, m ~ N(0, 1), v ~ U(0, 1)
    fresh     m = v = 0 (t = 1 only)
    tiny      g, m ~ 1e-9, v ~ 1e-18: den is eps
    cancel    b1 m = -(1 - b1) g (1 + 1e-3 N(0, 1)): m' is what is left of a cancellation
    zero_g    g = 0
    large     g, m ~ 1e4, v ~ 1e8
Layouts (element offsets, multiples of 64; `LAYOUTS`): small [0, 64, 1152, 1280] (the second workgroup starts inside
segment 1 and walks into segment 2), crowded (sixteen 64-element segments and one of 2112: a workgroup's 1024
elements span 16 segments; every third segment skipped, lr and wd differ per segment), long [0, 4160, 4224, 37568,
37632] (a 33344-element segment: two trips of the LARS norm loop, more than 32 workgroups; the end is no multiple of
1024), many (LARS only: 300 segments of 64 and 128, a second workgroup of lars_trust_kernel; matrices, vectors and
skipped segments mixed).
"""
import math

import torch
import torch.nn.functional as Fn

import ln_checks as lc
from ln_checks import EPS32, F64, F32, BF, k_from      # noqa: F401

ADAMW_CHECKS = ("adamw_m", "adamw_v", "adamw_p")
LARS_CHECKS = ("lars_mu", "lars_p")
CHECKS = ADAMW_CHECKS + LARS_CHECKS
BIT_CHECKS = ("lp", "untouched", "g", "pad_zero", "applied")
# worst error / (2^-24 mag) of the fp32 torch evaluation over the GPU module's case list (measure_k_ref)
K_REF_CPU = {"adamw_m": 2.138, "adamw_v": 3.468, "adamw_p": 3.714, "lars_mu": 4.578, "lars_p": 2.620}
K_REF_GPU = {"adamw_m": 2.138, "adamw_v": 3.468, "adamw_p": 3.714, "lars_mu": 4.578, "lars_p": 2.620}
K_REF = {n: max(K_REF_CPU.get(n, 0.0), K_REF_GPU.get(n, 0.0)) for n in CHECKS}
K = {name: k_from(v) for name, v in K_REF.items()}
BAND = 256              # guard elements on either side of every buffer handed to the library
TRUST = 1e-3


class Report(lc.Report):
    def __init__(self, tag="", measure=False, k=None):
        super().__init__(K if k is None else k, tag, measure)

    def bits(self, name, got, want, what):
        """bit for bit: lc.Report.same on the int views (a NaN equals itself, +0 and -0 differ)"""
        if self.measure:
            return
        self.worst.setdefault(name, 0.0)
        iv = {2: torch.int16, 4: torch.int32}[got.element_size()]
        if got.dtype != want.dtype or got.shape != want.shape:
            self.worst[name] = math.inf
            self.failed.append("%s %s: %s: %s %s, want %s %s" % (self.tag, name, what, got.dtype, tuple(got.shape),
                                                                 want.dtype, tuple(want.shape)))
            return
        self.same(name, got.contiguous().view(iv), want.contiguous().view(iv), what)


def f32r(x):
    """x as the ABI carries it: rounded to fp32, then a double"""
    return float(torch.tensor(float(x), dtype=F32))


def _gen(*key):
    seed = 2468
    for i, k in enumerate(key):
        seed = (seed * 1000003 + int(k) * (7919 + 2 * i)) % (2 ** 31 - 1)
    return torch.Generator("cpu").manual_seed(seed)


# ------------------------------------------------------------------ layouts
def _crowded_start():
    return [64 * i for i in range(17)] + [1024 + 2112]


def _many_start():
    s = [0]
    for i in range(300):
        s.append(s[-1] + (64 if i % 2 == 0 else 128))
    return s


def _layout(name):
    """-> start [S + 1], lr [S] (< 0: skipped), wd [S], mat [S], tail {segment: length of its zero tail},
    zero_p / zero_d: LARS matrix segments whose p / whose g + wd p is all zero (the latter's wd entry is 0)"""
    if name == "small":
        return dict(start=[0, 64, 1152, 1280], lr=[1e-2, 2e-2, 5e-3], wd=[0.0, 0.05, 0.1], mat=[0, 1, 1],
                    tail={1: 23}, zero_p=(), zero_d=())
    if name == "small_skip":        # the layout of tests/test_gpu_optim.py with its middle segment skipped
        return dict(start=[0, 64, 1152, 1280], lr=[1e-2, -1.0, 5e-3], wd=[0.01, 0.05, 0.1], mat=[1, 1, 0],
                    tail={0: 5}, zero_p=(), zero_d=())
    if name == "crowded":
        S = 17
        lr = [-1.0 if s % 3 == 2 else 1e-2 * (1 + s % 5) for s in range(S)]
        wd = [0.02 * (s % 4) for s in range(S)]
        mat = [1 if s % 2 == 1 or s == 16 or s == 4 else 0 for s in range(S)]
        wd[4] = 0.0
        return dict(start=_crowded_start(), lr=lr, wd=wd, mat=mat, tail={16: 40, 6: 7}, zero_p=(3,), zero_d=(4,))
    if name == "long":
        return dict(start=[0, 4160, 4224, 37568, 37632], lr=[1e-2, -1.0, 2e-2, 5e-3], wd=[0.05, 0.3, 0.05, 0.0],
                    mat=[1, 1, 1, 1], tail={0: 50, 2: 9}, zero_p=(3,), zero_d=())
    if name == "many":
        S = 300
        lr = [-1.0 if s % 7 == 3 else 0.05 * (1 + s % 3) for s in range(S)]
        wd = [0.01 * (1 + s % 4) for s in range(S)]
        mat = [1 if s % 3 != 1 else 0 for s in range(S)]
        for s in (260, 284):
            wd[s] = 0.0
        return dict(start=_many_start(), lr=lr, wd=wd, mat=mat, tail={5: 3, 299: 31}, zero_p=(9, 270), zero_d=(260, 284))
    raise KeyError(name)


LAYOUTS = {n: _layout(n) for n in ("small", "small_skip", "crowded", "long", "many")}
ADAMW_LAYOUTS = ("small", "small_skip", "crowded", "long")
LARS_LAYOUTS = ("small", "small_skip", "crowded", "long", "many")
for _n, _l in LAYOUTS.items():
    assert all(o % 64 == 0 for o in _l["start"]) and _l["start"][-1] <= 200 * 1024, _n
    assert all(_l["lr"][s] >= 0 and _l["mat"][s] for s in _l["zero_p"] + _l["zero_d"]), _n
    assert all(_l["wd"][s] == 0 for s in _l["zero_d"]) and all(_l["lr"][s] >= 0 for s in _l["tail"]), _n


def seg_index(start):
    lens = torch.tensor([b - a for a, b in zip(start[:-1], start[1:])])
    return torch.repeat_interleave(torch.arange(len(lens)), lens)


def _tail_ranges(lay):
    return [(lay["start"][s + 1] - t, lay["start"][s + 1]) for s, t in sorted(lay["tail"].items())]


# ------------------------------------------------------------------ AdamW: cases
ADAMW_FAMILIES = ("gauss", "fresh", "tiny", "cancel", "zero_g", "large")
BETAS = ((0.9, 0.95), (0.9, 0.999))
STEPS = (1, 2, 7, 1000, 100000)
EPSES = (1e-8, 1e-6)
COEFS = (1.0, 0.37)


def adamw_hypers():
    """(b1, b2, t, eps, mode, ctl[1]): not the full product; every t, eps and ctl[1] with both beta pairs, every t and
    eps with both counting modes"""
    out = []
    for bi, (b1, b2) in enumerate(BETAS):
        for ti, t in enumerate(STEPS):
            for mi, mode in enumerate(("host", "dev")):
                out.append((b1, b2, t, EPSES[(ti + mi + bi) % 2], mode, COEFS[(ti + bi) % 2] if mode == "dev" else 1.0))
    return out


def adamw_case(layout, family, hyper, lo=None, hi=None, seed=0):
    lay = LAYOUTS[layout]
    b1, b2, t, eps, mode, coef = hyper
    start = lay["start"]
    n = start[-1]
    g = _gen(1, seed, ADAMW_LAYOUTS.index(layout), ADAMW_FAMILIES.index(family), t, int(b2 * 1000), mode == "dev")
    rn = lambda: torch.randn(n, generator=g)
    p, gr, m, v = rn(), rn(), rn(), torch.rand(n, generator=g)
    if family == "fresh":
        assert t == 1
        m, v = torch.zeros(n), torch.zeros(n)
    elif family == "tiny":
        gr, m, v = 1e-9 * gr, 1e-9 * m, 1e-18 * v
    elif family == "cancel":
        m = (-(1 - f32r(b1)) / f32r(b1) * gr.double() * (1 + 1e-3 * rn().double())).float()
    elif family == "zero_g":
        gr = torch.zeros(n)
    elif family == "large":
        gr, m, v = 1e4 * gr, 3e3 * m, 1e8 * v
    seg = seg_index(start)
    lr = torch.tensor(lay["lr"], dtype=F32)
    gr = torch.where(lr[seg] < 0, torch.tensor(float("nan")), gr)      # stale values: not read
    for a, b in _tail_ranges(lay):
        p[a:b], gr[a:b], m[a:b], v[a:b] = 0.0, 0.0, 0.0, 0.0
    return {"kind": "adamw", "layout": layout, "family": family, "start": start, "lr": lr,
            "wd": torch.tensor(lay["wd"], dtype=F32), "b1": b1, "b2": b2, "eps": eps, "t": t, "mode": mode, "coef": coef,
            "lo": 0 if lo is None else lo, "hi": n if hi is None else hi, "pad": _tail_ranges(lay),
            "p": p, "g": gr, "m": m, "v": v, "lp": p.to(BF)}


def adamw_tag(c):
    return "adamw %s %s b2=%g t=%d eps=%g %s c=%g [%d, %d)" % (c["layout"], c["family"], c["b2"], c["t"], c["eps"],
                                                               c["mode"], c["coef"], c["lo"], c["hi"])


def _active(c):
    """elements an update is applied to, and the per-element lr and wd (0 where none is)"""
    seg = seg_index(c["start"])
    lr, wd = c["lr"].to(F64)[seg], c["wd"].to(F64)[seg]
    idx = torch.arange(c["start"][-1])
    act = (lr >= 0) & (idx >= c["lo"]) & (idx < c["hi"])
    zero = torch.zeros((), dtype=F64)
    return act, torch.where(act, lr, zero), torch.where(act, wd, zero), seg


# ------------------------------------------------------------------ AdamW: fp64 reference and checks
def adamw_ref(c, double_betas=False):
    act, lr, wd, _ = _active(c)
    r = (lambda x: float(x)) if double_betas else f32r
    b1, b2, eps, t = r(c["b1"]), r(c["b2"]), f32r(c["eps"]), c["t"]
    coef = f32r(c["coef"]) if c["mode"] == "dev" else 1.0
    p, m, v = c["p"].to(F64), c["m"].to(F64), c["v"].to(F64)
    g1 = coef * torch.where(act, c["g"].to(F64), torch.zeros((), dtype=F64))
    tm, tg = b1 * m, (1 - b1) * g1
    m1, mag_m = tm + tg, tm.abs() + tg.abs()
    v1 = b2 * v + (1 - b2) * g1 * g1
    bc1, bc2 = 1 - b1 ** t, 1 - b2 ** t
    den = v1.sqrt() / math.sqrt(bc2) + eps
    upd = (lr / bc1) * m1 / den
    return {"act": act, "m": m1, "mag_m": mag_m, "v": v1, "mag_v": v1, "upd": upd,
            "p": p * (1 - lr * wd) - upd, "mag_p": p.abs() + (lr / bc1) * mag_m / den,
            "slack_p": upd.abs() * 2 * EPS32 * (b1 ** t / bc1 + 0.5 * b2 ** t / bc2)}


def _unchanged(rep, c, o, names, keep, what):
    for name in names:
        rep.bits("untouched", o[name][keep], c[name][keep], "%s: %s" % (name, what))


def _pads(rep, c, o, names, act):
    for a, b in c["pad"]:
        if bool(act[a:b].all()):
            for name in names:
                rep.bits("pad_zero", o[name][a:b], torch.zeros(b - a), "%s: the zero tail [%d, %d) is not +0" % (name, a, b))


def adamw_check(c, o, rep):
    """o: p, m, v (fp32), lp (bf16) and g after the call, whole arena, on the CPU"""
    r = adamw_ref(c)
    act = r["act"]
    if bool(act.any()):
        rep.ratio("adamw_m", o["m"][act], r["m"][act], r["mag_m"][act])
        rep.ratio("adamw_v", o["v"][act], r["v"][act], r["mag_v"][act])
        rep.ratio("adamw_p", o["p"][act], r["p"][act], r["mag_p"][act], slack=r["slack_p"][act])
    rep.bits("lp", o["lp"][act], o["p"].to(BF)[act], "not the updated p rounded to bf16")
    _unchanged(rep, c, o, ("p", "m", "v", "lp"), ~act, "written in a skipped segment or outside [lo, hi)")
    rep.bits("g", o["g"], c["g"], "the gradient was written")
    _pads(rep, c, o, ("p", "m", "v"), act)
    return r


# ------------------------------------------------------------------ AdamW: the same formulae in plain fp32 torch
# name -> (optimizer, the check that must catch it)
MUTATIONS = {
    "coupled_decay": ("adamw", "adamw_p"),                  # g + wd p into the moments, no p (1 - lr wd)
    "decay_after_update": ("adamw", "adamw_p"),             # (p - upd) (1 - lr wd)
    "eps_inside_sqrt": ("adamw", "adamw_p"),                # sqrt(v' + eps)
    "eps_before_bias_correction": ("adamw", "adamw_p"),     # (sqrt(v') + eps) / sqrt(bc2)
    "bc2_outside_sqrt": ("adamw", "adamw_p"),               # sqrt(v') / bc2
    "t_off_by_one": ("adamw", "adamw_p"),
    "b2_for_m": ("adamw", "adamw_m"),
    "coef_missing_in_v": ("adamw", "adamw_v"),              # v' from the unclipped gradient
    "neighbour_lr": ("adamw", "adamw_p"),                   # a segment's first four elements take the previous lr
    "lp_truncated": ("adamw", "lp"),
    "lp_from_old_p": ("adamw", "lp"),
    "write_into_skipped": ("adamw", "untouched"),
    "wd_on_vector": ("lars", "lars_mu"),
    "q_on_vector": ("lars", "lars_mu"),
    "q_from_g_norm": ("lars", "lars_mu"),                   # |g| instead of |g + wd p|
    "norm_first_32768_only": ("lars", "lars_mu"),           # the second trip of the strided loop dropped
    "zero_norm_gives_0": ("lars", "lars_mu"),
    "momentum_on_dp": ("lars", "lars_mu"),                  # momentum (mu + dp)
    "p_minus_lr_dp": ("lars", "lars_p"),
    "lars_write_into_skipped": ("lars", "untouched"),
}


def _truncate_bf16(t):
    return (t.contiguous().view(torch.int32) & -65536).view(F32).to(BF)


def adamw_eval(c, mut=None, device="cpu", dt=F32):
    """the step in `dt` in the kernel's order of operations; `mut`: one of MUTATIONS"""
    act, lr64, wd64, seg = _active(c)
    if mut == "neighbour_lr":
        for s in range(1, len(c["start"]) - 1):
            if float(c["lr"][s - 1]) >= 0:
                lr64[c["start"][s]:c["start"][s] + 4] = float(c["lr"][s - 1])
        lr64 = torch.where(act, lr64, torch.zeros((), dtype=F64))
    T = lambda x: torch.tensor(float(x), dtype=F32).to(device=device, dtype=dt)
    on = lambda x: x.to(device=device, dtype=dt)
    actd = act.to(device)
    lr, wd = on(lr64.to(F32)), on(wd64.to(F32))
    b1, b2, eps = T(c["b1"]), T(c["b2"]), T(c["eps"])
    t = T(c["t"] + (1 if mut == "t_off_by_one" else 0))
    one = T(1.0)
    bc1, bc2 = one - torch.pow(b1, t), one - torch.pow(b2, t)
    rs = one / torch.sqrt(bc2)
    p, m, v = on(c["p"]), on(c["m"]), on(c["v"])
    g0 = torch.where(actd, on(c["g"]), torch.zeros((), dtype=dt, device=device))
    g = g0 * T(c["coef"]) if c["mode"] == "dev" else g0
    x = p * (one - lr * wd)
    if mut == "coupled_decay":
        g, x = g + wd * p, p
    mj = (b2 if mut == "b2_for_m" else b1) * m + (one - (b2 if mut == "b2_for_m" else b1)) * g
    gv = g0 if mut == "coef_missing_in_v" else g
    vj = b2 * v + (one - b2) * gv * gv
    if mut == "eps_inside_sqrt":
        den = torch.sqrt(vj + eps) * rs
    elif mut == "eps_before_bias_correction":
        den = (torch.sqrt(vj) + eps) * rs
    elif mut == "bc2_outside_sqrt":
        den = torch.sqrt(vj) / bc2 + eps
    else:
        den = torch.sqrt(vj) * rs + eps
    upd = (lr / bc1) * mj / den
    x = (p - upd) * (one - lr * wd) if mut == "decay_after_update" else x - upd
    keep = lambda new, old: torch.where(actd, new, on(old)).to(F32).cpu()
    o = {"p": keep(x, c["p"]), "m": keep(mj, c["m"]), "v": keep(vj, c["v"]), "g": c["g"].clone()}
    src = c["p"] if mut == "lp_from_old_p" else o["p"]
    o["lp"] = torch.where(act, _truncate_bf16(src) if mut == "lp_truncated" else src.to(BF), c["lp"])
    if mut == "write_into_skipped":
        sk = ~act & (torch.arange(act.numel()) >= c["lo"]) & (torch.arange(act.numel()) < c["hi"])
        o["m"] = torch.where(sk, c["m"] * 0.9, o["m"])
    return o


# ------------------------------------------------------------------ LARS: cases
LARS_FAMILIES = ("gauss", "zero_g", "large")
LARS_HYPERS = ((1e-2, 0.9), (0.0, 0.9), (1e-6, 0.0))       # (wd, momentum); the layout's wd table is scaled by wd / 1e-2


def lars_case(layout, family, hyper, mu_zero, sub=None, seed=0):
    """sub = (i0, i1): the call gets the segments [i0, i1) only, with seg_start rebased to their first element"""
    lay = LAYOUTS[layout]
    wd0, momentum = hyper
    start = lay["start"]
    n, S = start[-1], len(start) - 1
    g = _gen(2, seed, LARS_LAYOUTS.index(layout), LARS_FAMILIES.index(family), int(wd0 * 1e7), mu_zero)
    rn = lambda: torch.randn(n, generator=g)
    p, gr, mu = rn(), rn(), torch.zeros(n) if mu_zero else rn()
    if family == "zero_g":
        gr = torch.zeros(n)
    elif family == "large":
        gr = 1e4 * gr
    seg = seg_index(start)
    lr = torch.tensor(lay["lr"], dtype=F32)
    inside = lambda ss: torch.isin(seg, torch.tensor(list(ss), dtype=torch.long))
    p = torch.where(inside(lay["zero_p"]), torch.zeros(()), p)
    gr = torch.where(inside(lay["zero_d"]), torch.zeros(()), gr)
    gr = torch.where(lr[seg] < 0, torch.tensor(float("nan")), gr)
    for a, b in _tail_ranges(lay):
        p[a:b], gr[a:b], mu[a:b] = 0.0, 0.0, 0.0
    i0, i1 = (0, S) if sub is None else sub
    return {"kind": "lars", "layout": layout, "family": family, "start": start, "lr": lr,
            "wd": torch.tensor([w * wd0 / 1e-2 for w in lay["wd"]], dtype=F32), "mat": torch.tensor(lay["mat"], dtype=F32),
            "momentum": momentum, "trust": TRUST, "i0": i0, "i1": i1, "lo": start[i0], "hi": start[i1],
            "pad": _tail_ranges(lay), "p": p, "g": gr, "mu": mu}


def lars_tag(c):
    return "lars %s %s wd=%g mom=%g mu%s segments [%d, %d)" % (c["layout"], c["family"], float(c["wd"].max()),
                                                                c["momentum"], "=0" if not bool(c["mu"].any()) else "",
                                                                c["i0"], c["i1"])


# ------------------------------------------------------------------ LARS: fp64 reference and checks
def lars_ref(c):
    act, lr, wd, seg = _active(c)
    S = len(c["start"]) - 1
    mat = (c["mat"] != 0)[seg] & act
    momentum, trust = f32r(c["momentum"]), f32r(c["trust"])
    zero = torch.zeros((), dtype=F64)
    p, mu = c["p"].to(F64), c["mu"].to(F64)
    g = torch.where(act, c["g"].to(F64), zero)
    wdp = torch.where(mat, wd * p, zero)
    d = g + wdp
    pn = torch.zeros(S, dtype=F64).index_add_(0, seg[mat], p[mat] ** 2).sqrt()
    un = torch.zeros(S, dtype=F64).index_add_(0, seg[mat], d[mat] ** 2).sqrt()
    q = torch.where((pn > 0) & (un > 0), trust * pn / un.clamp_min(1e-300), torch.ones((), dtype=F64))
    qe = torch.where(mat, q[seg], torch.ones((), dtype=F64))
    mu1 = momentum * mu + d * qe
    mag_mu = (momentum * mu).abs() + (g.abs() + wdp.abs()) * qe
    return {"act": act, "q": q, "mu": mu1, "mag_mu": mag_mu, "p": p - lr * mu1, "mag_p": p.abs() + lr * mag_mu}


def lars_check(c, o, rep):
    """o: p, mu and g after the call, whole arena, on the CPU"""
    r = lars_ref(c)
    act = r["act"]
    if bool(act.any()):
        rep.ratio("lars_mu", o["mu"][act], r["mu"][act], r["mag_mu"][act])
        rep.ratio("lars_p", o["p"][act], r["p"][act], r["mag_p"][act])
    _unchanged(rep, c, o, ("p", "mu"), ~act, "written in a skipped segment or outside the range")
    rep.bits("g", o["g"], c["g"], "the gradient was written")
    _pads(rep, c, o, ("p", "mu"), act)
    return r


# ------------------------------------------------------------------ LARS: the same formulae in plain fp32 torch
def kernel_order_sumsq(x):
    """sum of x^2 over the last axis (a multiple of 4 long) in the order of lars_norm_partial_kernel +
    lars_trust_kernel; x [n] or [B, n]: B segments of one length at once"""
    lead = x.shape[:-1]
    x = x.reshape(-1, x.shape[-1])
    B, n = x.shape
    parts, trips = (-(-n // 1024), 1) if n <= 32768 else (32, -(-n // 32768))      # unused parts add +0: exact
    sq = Fn.pad(x, (0, trips * parts * 1024 - n)).view(B, trips, parts, 256, 4)
    sq = sq * sq
    a = torch.zeros(B, parts, 256, dtype=x.dtype, device=x.device)
    for k in range(trips):
        for j in range(4):
            a = a + sq[:, k, :, :, j]               # each thread's running sum
    w = a.view(B, parts, 4, 64)
    for o in (32, 16, 8, 4, 2, 1):                  # the wave tree: lane l adds lane l ^ o
        w = w[..., :o] + w[..., o:2 * o]
    w = w[..., 0]
    blk = ((w[..., 0] + w[..., 1]) + w[..., 2]) + w[..., 3]
    tot = torch.zeros(B, dtype=x.dtype, device=x.device)
    for k in range(parts):
        tot = tot + blk[:, k]
    return tot.reshape(lead)


def lars_eval(c, mut=None, device="cpu", dt=F32):
    act, lr64, wd64, seg = _active(c)
    T = lambda x: torch.tensor(float(x), dtype=F32).to(device=device, dtype=dt)
    on = lambda x: x.to(device=device, dtype=dt)
    actd = act.to(device)
    start, S = c["start"], len(c["start"]) - 1
    lr, wd_all = on(lr64.to(F32)), on(wd64.to(F32))
    is_mat = (c["mat"] != 0)
    matd = (is_mat[seg] & act).to(device)
    zero, one = T(0.0), T(1.0)
    momentum, trust = T(c["momentum"]), T(c["trust"])
    p, mu = on(c["p"]), on(c["mu"])
    g = torch.where(actd, on(c["g"]), zero)
    wd = wd_all if mut == "wd_on_vector" else torch.where(matd, wd_all, zero)
    d = g + wd * p
    q = torch.ones(S, dtype=dt, device=device)
    by_len = {}                                     # segments of one length go through the sums together
    for s in range(c["i0"], c["i1"]):
        if float(c["lr"][s]) >= 0 and (bool(is_mat[s]) or mut == "q_on_vector"):
            n = start[s + 1] - start[s]
            by_len.setdefault(min(n, 32768) if mut == "norm_first_32768_only" else n, []).append(s)
    for n, ss in by_len.items():
        idx = (torch.tensor([start[s] for s in ss]).view(-1, 1) + torch.arange(n).view(1, -1)).to(device)
        pn = torch.sqrt(kernel_order_sumsq(p[idx]))
        un = torch.sqrt(kernel_order_sumsq((g if mut == "q_from_g_norm" else d)[idx]))
        ok = (pn > 0) & (un > 0)
        q[torch.tensor(ss, device=device)] = torch.where(ok, trust * pn / torch.where(ok, un, one),
                                                         zero if mut == "zero_norm_gives_0" else one)
    dp = d * q[seg.to(device)]
    mu1 = momentum * (mu + dp) if mut == "momentum_on_dp" else momentum * mu + dp
    p1 = p - lr * (dp if mut == "p_minus_lr_dp" else mu1)
    keep = lambda new, old: torch.where(actd, new, on(old)).to(F32).cpu()
    o = {"p": keep(p1, c["p"]), "mu": keep(mu1, c["mu"]), "g": c["g"].clone()}
    if mut == "lars_write_into_skipped":
        idx = torch.arange(act.numel())
        sk = ~act & (idx >= c["lo"]) & (idx < c["hi"])
        o["mu"] = torch.where(sk, c["mu"] * 0.9, o["mu"])
    return o


# ------------------------------------------------------------------ table
KINDS = {"adamw": (adamw_case, adamw_eval, adamw_check, adamw_tag), "lars": (lars_case, lars_eval, lars_check, lars_tag)}


def make(kind, args):
    return KINDS[kind][0](*args)


def evaluate(c, mut=None, device="cpu"):
    return KINDS[c["kind"]][1](c, mut if mut is not None and MUTATIONS[mut][0] == c["kind"] else None, device)


def run_check(c, o, tag="", measure=False, k=None):
    rep = Report(tag or KINDS[c["kind"]][3](c), measure, k)
    KINDS[c["kind"]][2](c, o, rep)
    return rep


# ------------------------------------------------------------------ the case list of the GPU module
def _adamw_ranges(layout):
    """[lo, hi) of the calls besides the whole arena: each segment alone, and [64, end) — the workgroups then no
    longer start at multiples of 1024 of the arena ([1152, 1280) on small is its last segment alone)"""
    start = LAYOUTS[layout]["start"]
    return list(zip(start[:-1], start[1:])) + [(64, start[-1])]


def gpu_specs(kind):
    """(group, arguments of the kind's case constructor) of every case tests/test_gpu_optim_kernels.py runs"""
    out = []
    if kind == "adamw":
        hypers = adamw_hypers()
        for layout in ADAMW_LAYOUTS:
            for fi, family in enumerate(ADAMW_FAMILIES):
                for hi_, h in enumerate(hypers):
                    if family == "fresh" and h[2] != 1:
                        continue
                    # the long arena with a third of the hyper-parameter list per family, the others with all of it
                    if layout == "long" and family != "fresh" and (hi_ + fi) % 3:
                        continue
                    out.append(("%s-%s" % (layout, family), (layout, family, h)))
            # ranges: two host-counted and two device-counted hyper-parameter sets, one with ctl[1] = 0.37
            picks = [h for h in hypers if (h[2], h[4]) in ((7, "host"), (2, "dev"))]
            for lo, hi in _adamw_ranges(layout):
                for j, h in enumerate(picks):
                    out.append(("%s-ranges" % layout, (layout, ("gauss", "cancel")[j % 2], h, lo, hi)))
    elif kind == "lars":
        for layout in LARS_LAYOUTS:
            for family in LARS_FAMILIES:
                for h in LARS_HYPERS:
                    for mu_zero in (False, True):
                        out.append(("%s-%s" % (layout, family), (layout, family, h, mu_zero)))
        # a sub-range of the arena with seg_start rebased to it
        for layout, sub in (("crowded", (2, 17)), ("crowded", (1, 9)), ("long", (1, 4)), ("long", (2, 3)), ("many", (7, 290)),
                            ("small", (1, 2))):
            for h in LARS_HYPERS:
                out.append(("%s-sub" % layout, (layout, "gauss", h, False, sub)))
    return out


def groups(specs):
    return list(dict.fromkeys(s[0] for s in specs))


def measure_k_ref(device, log=print):
    """worst error / (2^-24 mag) per bounded check of the fp32 torch evaluation on `device` over the GPU module's
    case list"""
    worst = {}
    for kind in KINDS:
        for grp, a in gpu_specs(kind):
            c = make(kind, a)
            rep = run_check(c, evaluate(c, device=device), measure=True)
            for n, v in rep.worst.items():
                if n in CHECKS and v > worst.get(n, 0.0):
                    worst[n] = v
                    log("k_ref %s = %.3f at %s" % (n, v, rep.tag))
    return worst


def beta_rounding_deviation(n=4096):
    """{(b1, b2): {t: worst |upd(fp32-rounded betas) - upd(double betas)| / |upd|}}, both in fp64: what the ABI's
    float betas cost against torch.optim.AdamW.  Not a check of the kernels."""
    out = {}
    for b1, b2 in BETAS:
        out[(b1, b2)] = {}
        g = _gen(3, int(b2 * 1000))
        beta = ((f32r(b1), f32r(b2)), (b1, b2))
        m = [torch.zeros(n, dtype=F64) for _ in beta]
        v = [torch.zeros(n, dtype=F64) for _ in beta]
        for t in range(1, 1001):                    # t steps from m = v = 0 on the same gaussian gradients
            gr = torch.randn(n, generator=g, dtype=F64)
            upd = []
            for i, (a, b) in enumerate(beta):
                m[i] = a * m[i] + (1 - a) * gr
                v[i] = b * v[i] + (1 - b) * gr * gr
                upd.append(m[i] / (1 - a ** t) / (v[i].sqrt() / math.sqrt(1 - b ** t) + 1e-8))
            if t in (1, 10, 1000):
                big = upd[1].abs() > 1e-2 * upd[1].abs().max()      # relative to an update that is not a cancellation
                out[(b1, b2)][t] = float(((upd[0] - upd[1]).abs() / upd[1].abs())[big].max())
    return out


# ------------------------------------------------------------------ a case on the library (the only GPU code besides
# measure_k_ref(device))
def _banded(t, device):
    """t in the middle of a buffer with BAND poisoned elements on either side -> (buffer, view)"""
    fill = torch.full((BAND,), 12288.0, dtype=t.dtype)
    buf = torch.cat([fill, t, fill]).to(device)
    return buf, buf[BAND:BAND + t.numel()]


def _bands_ok(rep, bufs):
    for name, (buf, _) in bufs.items():
        n = buf.numel() - 2 * BAND
        want = torch.full((BAND,), 12288.0, dtype=buf.dtype)
        rep.bits("untouched", buf[:BAND].cpu(), want, "%s: written before the buffer" % name)
        rep.bits("untouched", buf[BAND + n:].cpu(), want, "%s: written past the buffer" % name)


def run_adamw(c, device="cuda"):
    """the case through ssl4gie_adamw_arena -> (outputs on the CPU, a Report holding the guard bands' and the
    counter's checks)"""
    from ssl4gie_amd import _lib
    from ssl4gie_amd.ops import ptr, stream
    bufs = {k: _banded(c[k], device) for k in ("p", "g", "m", "v", "lp")}
    S = len(c["start"]) - 1
    start = torch.tensor(c["start"], dtype=torch.int64, device=device)
    lr, wd = c["lr"].to(device), c["wd"].to(device)
    dev = c["mode"] == "dev"
    applied = torch.tensor([c["t"] - 1], dtype=torch.int32, device=device) if dev else None
    ctl = torch.tensor([0.0, c["coef"], 0.0, 0.0], dtype=F32, device=device) if dev else None
    v = {k: b[1] for k, b in bufs.items()}
    _lib.check(_lib.load().ssl4gie_adamw_arena(
        ptr(v["p"]), ptr(v["g"]), ptr(v["m"]), ptr(v["v"]), ptr(start), ptr(lr), ptr(wd), S, c["b1"], c["b2"], c["eps"],
        0 if dev else c["t"], ptr(applied), c["lo"], c["hi"], ptr(v["lp"]), ptr(ctl), 0, int(dev), stream()), "adamw_arena")
    torch.cuda.synchronize()
    rep = Report(adamw_tag(c))
    _bands_ok(rep, bufs)
    if dev:
        rep.bits("applied", applied.cpu(), torch.tensor([c["t"]], dtype=torch.int32), "the counter did not advance by one")
        rep.bits("applied", ctl.cpu(), torch.tensor([0.0, c["coef"], 0.0, 0.0]), "the control block was written")
    return {k: b.cpu() for k, b in v.items()}, rep


def run_lars(c, device="cuda"):
    """the case through ssl4gie_lars_arena, which gets the segments [i0, i1) behind pointers moved to their first
    element and a seg_start rebased to it"""
    from ssl4gie_amd import _lib
    from ssl4gie_amd.ops import ptr, stream
    L = _lib.load()
    bufs = {k: _banded(c[k], device) for k in ("p", "g", "mu")}
    i0, i1, lo, hi = c["i0"], c["i1"], c["lo"], c["hi"]
    S = i1 - i0
    start = torch.tensor([s - lo for s in c["start"][i0:i1 + 1]], dtype=torch.int64, device=device)
    lr, wd, mat = (c[k][i0:i1].contiguous().to(device) for k in ("lr", "wd", "mat"))
    ws = torch.full((L.ssl4gie_lars_workspace_bytes(S) // 4 + 2 * BAND,), 12288.0, dtype=F32, device=device)
    v = {k: b[1] for k, b in bufs.items()}
    _lib.check(L.ssl4gie_lars_arena(ptr(v["p"]) + 4 * lo, ptr(v["g"]) + 4 * lo, ptr(v["mu"]) + 4 * lo, ptr(start), ptr(lr),
                                    ptr(wd), ptr(mat), S, c["momentum"], c["trust"], ptr(ws) + 4 * BAND, hi - lo, stream()),
               "lars_arena")
    torch.cuda.synchronize()
    rep = Report(lars_tag(c))
    _bands_ok(rep, dict(bufs, workspace=(ws, None)))
    return {k: b.cpu() for k, b in v.items()}, rep
