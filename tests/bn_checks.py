"""fp64 reference of training-mode BatchNorm and the per-element / per-channel checks that pin the
`bn_*` kernels of resnet_ops.hip to it (tests/test_gpu_batchnorm_kernels.py; proof that the checks bite:
tests/test_bn_checks_cpu.py).

Reference (`ref_stats`, `ref_forward`, `ref_backward`): the textbook formulae in torch float64,
    mean = E[x], var = E[(x - mean)^2] (biased), rstd = (var + eps)^-1/2,
    y = act((x - mean) rstd gamma + beta (+ res)),
    running_mean <- (1 - m) running_mean + m mean, running_var <- (1 - m) running_var + m var n / (n - 1),
    g = mask ? dy : 0, dbeta = sum_r g, dgamma = sum_r g xhat, dres = g,
    dx = gamma rstd (g - inv_count sum_r g - xhat inv_count sum_r g xhat).

What is compared with what.  The statistics a kernel returns are compared per channel with the fp64 statistics
of x.  Every OTHER output is compared with the fp64 evaluation that starts from exactly what the kernel was
handed or returned in fp32: y from the (mean, rstd) the forward returned, the backward from the (mean, rstd,
ReLU mask) it was given.  An error of the statistics is therefore charged to the statistics check and nothing
else, and the backward's mask has no tie ambiguity (it is `y > 0` of the STORED output / the bit map).

Bounds: |got - ref| <= rho |ref| + k 2^-24 mag, per element or per channel, never a global max-norm.
  rho = 2^-8 for bf16 outputs (one final rounding), 0 for fp32 outputs and for every fp32 per-channel vector;
  mag = the fp64 sum of the ABSOLUTE values of the terms that are added:
    y         |x a| + |mean a| + |beta| + |res|, a = rstd gamma      (b = beta - mean a is itself a signed sum:
              its two terms enter separately; |b| alone is violated by a correct fp32 x a + b wherever beta
              and mean a cancel)
    dx        |a| (|g| + inv_count sum_r |g| + |xhat| inv_count sum_r |g xhat|)
    sum g     sum_r |g|;   sum g xhat: sum_r |g xhat|   (+ |initial value| with accumulate)
    mean      mean_r |x - x0|                 x0 = x[0, c], the kernels' pivot; 0 on the partials path;
              plus 2^-24 |mean| outside the factor k: mean = x0 + E[x - x0] is rounded once more at its own size
    var       mean_r (x - x0)^2 + (mean_r |x - x0|)^2
    rstd      rstd^3 / 2 (var's mag) + rstd   (propagated through (var + eps)^-1/2, plus its own rounding)
    running   m (the statistic's mag) (n / (n - 1)) + |(1 - m) old| + |m new|
  On the partials path (GEMM-epilogue sums about 0, var = E[x^2] - E[x]^2 in fp32) the statistics' mag is
  multiplied by (1 + mean^2 / var): the price of having no pivot, as a formula.  A constant channel has
  var = 0 there and the scale is infinite — the partials path promises nothing for it (the direct path does).

k.  Procedure: evaluate the same formulae in plain fp32 torch (`fp32_eval`: `sum(0)` reductions, pivoted sums
for the direct path and sums about 0 for the partials path; neither the kernels nor the engine), run it through
these checks over the case list of the GPU module (`measure_k_ref`), record the worst error / (2^-24 mag) per
check as k_ref, and set k = max(16, 4 k_ref) rounded up to a power of two (the 4 covers the kernels' longer
dependent-add chains, ~100 sequential adds per lane at the stem shape, against torch's blocked sums).
Measured k_ref (K_REF below) -> k (K below):

    check      k_ref   k        check      k_ref   k
    mean       23.73   128       y           3.94    16
    var        42.58   256       dx          4.67    32
    rstd       28.56   128       sums        4.01    32
    run_mean    3.59    16       dgamma      3.92    16
    run_var    12.20    64       dbeta       2.92    16

ReLU: the forward's `y > 0` must agree with the sign of the fp64 pre-activation except where
|pre| < k 2^-24 mag; at most MAX_TIE_SHARE of a case's elements may be excluded that way.  (rows = 1 runs without
ReLU: every channel is constant there, rstd = eps^-1/2 = 316 widens the radius to ~1e-3 and a few tenths of a
percent of the signs are undecidable; the exact-integer family covers the masks at one row.)
rows = 1: torch refuses the case; the engine's convention is that the unbiased factor n / (n - 1) is taken as 1
(the running variance is blended with the biased value, 0).  `ref_running` states it.
"""
import math

import torch

EPS32 = 2.0 ** -24
F64 = torch.float64
MAX_TIE_SHARE = 1e-3
CHECKS = ("mean", "var", "rstd", "run_mean", "run_var", "y", "dx", "sums", "dgamma", "dbeta")
# worst error / (2^-24 mag) of the fp32 torch evaluation over the case list (measure_k_ref; see the docstring):
# the larger of torch on the CPU (edge rows and partition shapes) and torch on the MI355X (the whole list).  The
# statistics' figures come from the production maps (802 816 x 48: mean 23.7, var 42.6, rstd 28.6 — torch's own
# device sums over ~10^6 rows); the kernels themselves measured mean 4.2, var 30.1, rstd 13.9, run_var 8.2, y 2.9,
# dx 5.0, sums 3.4, dgamma 3.8, dbeta 2.6 over the same list.
K_REF = {"mean": 23.734, "var": 42.575, "rstd": 28.56, "run_mean": 3.591, "run_var": 12.201, "y": 3.941, "dx": 4.666,
         "sums": 4.006, "dgamma": 3.919, "dbeta": 2.919}


def k_from(k_ref):
    return max(16, 2 ** math.ceil(math.log2(max(4.0 * k_ref, 1.0))))


K = {name: k_from(v) for name, v in K_REF.items()}


def rho(dtype):
    return 2.0 ** -8 if dtype == torch.bfloat16 else 0.0


class Report:
    """worst error / (2^-24 mag) per check, and the checks that exceeded their k"""

    def __init__(self, k=None, tag="", measure=False):
        self.k = K if k is None else k
        self.tag = tag
        self.measure = measure      # record the ratios, fail none (k_ref)
        self.worst = {}
        self.failed = []

    def ratio(self, name, got, ref, mag, rho_=0.0, kname=None, slack=0.0):
        got = got.to(F64)
        err = ((got - ref).abs() - rho_ * ref.abs() - slack).clamp_min(0)
        r = err / (EPS32 * mag)
        r = torch.where(err == 0, torch.zeros_like(r), r)           # 0 / 0: an exact value
        r = torch.nan_to_num(r, nan=math.inf, posinf=math.inf).reshape(-1)
        m, i = r.max(0)
        self.note(name, float(m), kname or name, "at flat index %d of shape %s" % (int(i), tuple(got.shape)))

    def note(self, name, value, kname, where=""):
        self.worst[name] = max(self.worst.get(name, 0.0), value)
        if not value <= self.k[kname] and not self.measure:
            self.failed.append("%s %s: error = %.4g x 2^-24 mag > k = %g %s" % (self.tag, name, value, self.k[kname], where))

    def fail(self, name, msg):
        if self.measure:
            return
        self.worst[name] = math.inf
        self.failed.append("%s %s: %s" % (self.tag, name, msg))

    def names(self):
        return sorted({f.split(":")[0].split()[-1] for f in self.failed})

    def assert_ok(self):
        assert not self.failed, "\n".join(self.failed)


# ------------------------------------------------------------------ fp64 reference
def ref_stats(x, pivot=True):
    """fp64 (mean, biased var) over the rows of x [rows, C] and the mags of their bounds: sums about
    x0 = x[0] (pivot) or about 0, the latter scaled by 1 + mean^2 / var"""
    xd = x.to(F64)
    d0 = xd - xd[0]          # the fp64 statistics themselves are taken about row 0: a constant channel is exactly
    dm = d0.mean(0)          # mean = x0, var = 0, whatever way torch forms a mean
    mean = xd[0] + dm
    var = ((d0 - dm) ** 2).mean(0)
    d = d0 if pivot else xd
    del xd, d0
    t_mean = d.abs().mean(0)
    t_var = (d * d).mean(0) + t_mean ** 2
    if not pivot:
        scale = 1.0 + torch.where(mean == 0, torch.zeros_like(mean), mean ** 2 / var)   # var == 0: inf
        t_mean, t_var = t_mean * scale, t_var * scale
    return {"mean": mean, "var": var, "t_mean": t_mean, "t_var": t_var, "n": x.shape[0]}


def unbiased_factor(n):
    return n / (n - 1.0) if n > 1 else 1.0    # rows = 1: the engine's convention (torch refuses the case)


def ref_running(st, rm0, rv0, momentum):
    u = unbiased_factor(st["n"])
    rm = (1 - momentum) * rm0.to(F64) + momentum * st["mean"]
    rv = (1 - momentum) * rv0.to(F64) + momentum * st["var"] * u
    m_rm = momentum * st["t_mean"] + ((1 - momentum) * rm0.to(F64)).abs() + (momentum * st["mean"]).abs()
    m_rv = momentum * u * st["t_var"] + ((1 - momentum) * rv0.to(F64)).abs() + momentum * st["var"] * u
    return rm, rv, m_rm, m_rv


def check_stats(rep, st, eps, mean=None, var=None, rstd=None, run=None, tag=""):
    """run = (got running_mean, got running_var, rm0, rv0, momentum)"""
    if mean is not None:
        rep.ratio(tag + "mean", mean, st["mean"], st["t_mean"], kname="mean", slack=EPS32 * st["mean"].abs())
    if var is not None:
        rep.ratio(tag + "var", var, st["var"], st["t_var"], kname="var")
    if rstd is not None:
        r = (st["var"] + eps) ** -0.5
        rep.ratio(tag + "rstd", rstd, r, 0.5 * r ** 3 * st["t_var"] + r, kname="rstd")
    if run is not None:
        rm, rv, m_rm, m_rv = ref_running(st, run[2], run[3], run[4])
        rep.ratio(tag + "run_mean", run[0], rm, m_rm, kname="run_mean")
        rep.ratio(tag + "run_var", run[1], rv, m_rv, kname="run_var")


def _col(v, like, fill):
    return torch.full((like.shape[1],), fill, dtype=F64, device=like.device) if v is None else v.to(F64)


def ref_forward(x, mean, rstd, gamma, beta, res):
    """fp64 pre-activation (x - mean) rstd gamma + beta (+ res) and the mag of its bound"""
    xd = x.to(F64)
    mean, rstd = mean.to(F64), rstd.to(F64)
    a = rstd * _col(gamma, x, 1.0)
    b = _col(beta, x, 0.0)
    pre = (xd - mean) * a + b
    mag = (xd * a).abs() + ((mean * a).abs() + b.abs())
    if res is not None:
        pre += res.to(F64)
        mag += res.to(F64).abs()
    return pre, mag


def check_forward(rep, x, mean, rstd, gamma, beta, res, relu, y, tag=""):
    """y against the fp64 evaluation from the (mean, rstd) the kernel returned or was given; with relu, the
    sign decisions against the fp64 pre-activation"""
    pre, mag = ref_forward(x, mean, rstd, gamma, beta, res)
    rep.ratio(tag + "y", y, pre.clamp_min(0) if relu else pre, mag, rho(y.dtype), kname="y")
    if relu:
        tie = pre.abs() < rep.k["y"] * EPS32 * mag
        wrong = ((y > 0) != (pre > 0)) & ~tie
        if bool(wrong.any()):
            rep.fail(tag + "y", "ReLU mask differs from the sign of the fp64 pre-activation at %d elements"
                     % int(wrong.sum()))
        share = float(tie.sum()) / tie.numel()
        rep.worst["tie_share"] = max(rep.worst.get("tie_share", 0.0), share)
        if share > MAX_TIE_SHARE:
            rep.fail(tag + "y", "%.3g of the elements excluded as ReLU ties (cap %g)" % (share, MAX_TIE_SHARE))


def ref_backward(dy, mask, x, mean, rstd, gamma, inv_count, sums=None):
    """fp64 backward from the handed (mean, rstd, mask [bool or None]); `sums` [2, C]: the (global) sums to form
    dx with instead of the local ones.  -> dict g, s1, s2, A1, A2, dx, mag_dx"""
    g = dy.to(F64)
    if mask is not None:
        g = torch.where(mask, g, torch.zeros_like(g))
    mean, rstd = mean.to(F64), rstd.to(F64)
    xhat = (x.to(F64) - mean) * rstd
    gx = g * xhat
    o = {"g": g, "s1": g.sum(0), "s2": gx.sum(0), "A1": g.abs().sum(0), "A2": gx.abs().sum(0)}
    del gx
    a = rstd * _col(gamma, x, 1.0)
    s1, s2, A1, A2 = o["s1"], o["s2"], o["A1"], o["A2"]
    if sums is not None:   # W identical ranks: the absolute sums scale as the signed ones do
        s1, s2 = sums[0].to(F64), sums[1].to(F64)
        w = round(1.0 / (inv_count * x.shape[0]))
        A1, A2 = A1 * w, A2 * w
    o["dx"] = a * (g - s1 * inv_count - xhat * (s2 * inv_count))
    o["mag_dx"] = a.abs() * (g.abs() + A1 * inv_count + xhat.abs() * (A2 * inv_count))
    return o


def check_backward(rep, bw, dtype, dx=None, dres=None, sums=None, dgamma=None, dbeta=None, dg0=None, db0=None,
                   tag=""):
    """bw = ref_backward(...); dg0 / db0: the values dgamma / dbeta held before an accumulating call"""
    if dx is not None:
        rep.ratio(tag + "dx", dx, bw["dx"], bw["mag_dx"], rho(dtype), kname="dx")
    if dres is not None and not torch.equal(dres.to(F64), bw["g"]):   # dy or 0: no rounding at all
        rep.fail(tag + "dres", "not the masked gradient at %d elements" % int((dres.to(F64) != bw["g"]).sum()))
    if sums is not None:
        rep.ratio(tag + "sums[0]", sums[0], bw["s1"], bw["A1"], kname="sums")
        rep.ratio(tag + "sums[1]", sums[1], bw["s2"], bw["A2"], kname="sums")
    if dbeta is not None:
        z = 0.0 if db0 is None else db0.to(F64)
        rep.ratio(tag + "dbeta", dbeta, bw["s1"] + z, bw["A1"] + abs(z), kname="dbeta")
    if dgamma is not None:
        z = 0.0 if dg0 is None else dg0.to(F64)
        rep.ratio(tag + "dgamma", dgamma, bw["s2"] + z, bw["A2"] + abs(z), kname="dgamma")


# ------------------------------------------------------------------ cases
def make_case(rows, C, dtype, device, seed, relu=True, with_res=True, affine=True):
    """real-valued inputs, generated on `device`: per-channel scale in [0.5, 2] and offset ~ N(0, 1);
    channel 0: mean = +8 sigma, 5: mean = -8 sigma, 3: constant (variance exactly 0);
    gamma ~ N(0, 1) with channel 1: gamma = beta = 0 (y exactly 0), 2: gamma = 0, 4: gamma < 0"""
    g = torch.Generator(device).manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=g, device=device)
    sig = 0.5 + 1.5 * torch.rand(C, generator=g, device=device)
    mu = rn(C)
    mu[0], mu[5] = 8 * sig[0], -8 * sig[5]
    x = rn(rows, C).mul_(sig).add_(mu)
    x[:, 3] = 1.5
    c = {"rows": rows, "C": C, "dtype": dtype, "relu": relu, "eps": 1e-5, "momentum": 0.1,
         "x": x.to(dtype), "res": rn(rows, C).to(dtype) if with_res else None, "dy": rn(rows, C).to(dtype),
         "gamma": None, "beta": None,
         "rm0": rn(C), "rv0": 0.5 + torch.rand(C, generator=g, device=device),
         "dg0": rn(C), "db0": rn(C)}
    if affine:
        gamma, beta = rn(C), 0.3 * rn(C)
        gamma[1], beta[1] = 0.0, 0.0
        gamma[2], beta[2] = 0.0, 0.25
        gamma[4] = -gamma[4].abs() - 0.1
        c["gamma"], c["beta"] = gamma, beta
    return c


def partials_of(x, block=128):
    """what a GEMM epilogue hands over: per `block` rows (sum x, sum x^2) about 0, [parts, 2, C] fp32 (each partial
    correctly rounded from fp64)"""
    rows, C = x.shape
    pad = (-rows) % block
    xd = x.to(F64)
    if pad:
        xd = torch.cat([xd, xd.new_zeros(pad, C)])
    xd = xd.view(-1, block, C)
    return torch.stack([xd.sum(1), (xd * xd).sum(1)], 1).float().contiguous()


# ------------------------------------------------------------------ the same formulae in plain fp32 torch
MUTATIONS = ("drop_row", "dup_row", "unbiased_norm", "mask_shift", "mask_ge", "dres_unmasked", "sum_x_not_xhat",
             "run_var_biased", "last_strip", "gamma_ignored")


def fp32_eval(c, pivot=True, mut=None, dt=torch.float32):
    """training-mode BatchNorm forward + backward of case `c` in `dt` with straightforward sum(0) reductions.
    `mut`: one of MUTATIONS — a deliberately wrong variant (tests/test_bn_checks_cpu.py)"""
    x, n, C = c["x"].to(dt), c["rows"], c["C"]
    one = lambda v, f: torch.full((C,), f, dtype=dt, device=x.device) if v is None else v.to(dt)
    gamma, beta = one(c["gamma"], 1.0), one(c["beta"], 0.0)
    if mut == "gamma_ignored":
        gamma = gamma.clone()
        gamma[6] = 1.0

    def rows_of(t):
        if mut == "drop_row":
            return t[:-1]
        if mut == "dup_row":
            return torch.cat([t, t[-1:]])
        return t
    x0 = x[0] if pivot else torch.zeros(C, dtype=dt, device=x.device)
    d = rows_of(x - x0)
    dm = d.sum(0) / n
    var = ((d * d).sum(0) / n - dm * dm).clamp_min(0)
    mean = x0 + dm
    u = unbiased_factor(n)
    rstd = torch.rsqrt((var * u if mut == "unbiased_norm" else var) + c["eps"])
    m = c["momentum"]
    o = {"mean": mean, "var": var, "rstd": rstd,
         "run_mean": (1 - m) * c["rm0"].to(dt) + m * mean,
         "run_var": (1 - m) * c["rv0"].to(dt) + m * (var if mut == "run_var_biased" else var * u)}
    y = (x - mean) * rstd * gamma + beta
    if c["res"] is not None:
        y = y + c["res"].to(dt)
    if c["relu"]:
        y = y.clamp_min(0)
    y = y.to(c["dtype"])
    dy = c["dy"].to(dt)
    g = dy
    if c["relu"]:
        mask = y >= 0 if mut == "mask_ge" else y > 0
        if mut == "mask_shift":
            mask = mask.reshape(-1).roll(1).view_as(mask)
        g = torch.where(mask, dy, torch.zeros_like(dy))
    xhat = (x - mean) * rstd
    s1 = rows_of(g).sum(0)
    s2 = rows_of(g * (x if mut == "sum_x_not_xhat" else xhat)).sum(0)
    dx = (rstd * gamma) * (g - s1 / n - xhat * (s2 / n))
    o.update(y=y, dx=dx.to(c["dtype"]), dres=(dy if mut == "dres_unmasked" else g).to(c["dtype"]),
             sums=torch.stack([s1, s2]), dbeta=c["db0"].to(dt) + s1, dgamma=c["dg0"].to(dt) + s2)
    if mut == "last_strip":
        for name in ("y", "dx", "dres"):
            o[name][:, -8:] = 0
    return o


def check_all(c, o, pivot=True, k=None, tag="", measure=False):
    """every check of this module on the outputs `o` (keys as fp32_eval returns them) of case `c`: the
    statistics against x, y from o's statistics, the backward from o's statistics and the mask of o's y"""
    rep = Report(k, tag, measure)
    st = ref_stats(c["x"], pivot)
    check_stats(rep, st, c["eps"], o["mean"], o["var"], o["rstd"],
                (o["run_mean"], o["run_var"], c["rm0"], c["rv0"], c["momentum"]))
    check_forward(rep, c["x"], o["mean"], o["rstd"], c["gamma"], c["beta"], c["res"], c["relu"], o["y"])
    bw = ref_backward(c["dy"], (o["y"] > 0) if c["relu"] else None, c["x"], o["mean"], o["rstd"], c["gamma"],
                      1.0 / c["rows"])
    check_backward(rep, bw, c["dtype"], o["dx"], o["dres"], o["sums"], o["dgamma"], o["dbeta"], c["dg0"], c["db0"])
    return rep


# ------------------------------------------------------------------ the case list of the GPU module
def lane_step(C, dtype):
    """rows a lane advances per step when the map is one partition (bn_lanes: 4 waves x rows per wave)"""
    cg = C // (8 if dtype == torch.bfloat16 else 4)
    lpr = cg if cg < 64 and not cg & (cg - 1) else 64
    return 4 * (64 // lpr)


EDGE_C = (8, 16, 32, 24, 48, 96, 192, 512, 520, 1032, 2048, 4096)


def edge_seed(rows, C):
    return 7919 * C + rows


def to_device(c, device):
    return {k: v.to(device) if torch.is_tensor(v) else v for k, v in c.items()}


def edge_case(rows, C, dtype, relu, with_res, affine):
    """a small case generated on the CPU, the same on every machine; with relu, the first seed whose fp32
    evaluation leaves out at most MAX_TIE_SHARE of the elements at twice the exclusion radius (a tiny map has
    no room for a single tie: 1 of 520 elements is already 0.19 %)"""
    for s in range(64):
        c = make_case(rows, C, dtype, "cpu", edge_seed(rows, C) + 1000003 * s, relu, with_res, affine)
        if not relu:
            return c
        o = fp32_eval(c)
        rep = Report({n: 2 * v for n, v in K.items()})
        check_forward(rep, c["x"], o["mean"], o["rstd"], c["gamma"], c["beta"], c["res"], True, o["y"])
        if rep.worst["tie_share"] <= MAX_TIE_SHARE:
            return c
    raise AssertionError("no seed keeps the ReLU ties of %d x %d within the cap" % (rows, C))


def edge_rows(C, dtype):
    s = lane_step(C, dtype)
    return [1, 2, 3] + [m * s + e for m in range(1, 6) for e in (-1, 0, 1) if m * s + e > 3]


# direct path: rows x C with 1, 31, 32, 33, 256, 257, 1024 partitions (one per 64 Ki elements; C <= 512)
PARTITION_SHAPES = ((128, 512, 1), (31 * 128, 512, 31), (32 * 128, 512, 32), (33 * 128 + 5, 512, 33),
                    (256 * 256 + 3, 256, 256), (257 * 1024, 64, 257), (1024 * 256 + 77, 256, 1024))
# hand-made partial counts: 256-thread tail without / with its eight-deep unroll (29: wave 0 alone, 32: all four
# waves), 1024-thread tail (> 256), fold (> 2048) without / with a remainder
PARTIAL_COUNTS = (1, 3, 28, 29, 31, 32, 33, 64, 255, 256, 257, 384, 2047, 2048, 2049, 6272, 25088)
# one 256-image view (conv-stem: batch 64), bf16: (rows, C, affine)
PRODUCTION = ((3211264, 64, True), (802816, 64, True), (802816, 128, True), (802816, 256, True),
              (200704, 128, True), (200704, 256, True), (200704, 512, True), (50176, 256, True),
              (50176, 512, True), (50176, 1024, True), (12544, 512, True), (12544, 2048, True),
              (256, 4096, True), (256, 256, False), (1024, 8192, False), (802816, 48, True), (200704, 96, True))


def bn_parts(rows, C):
    """partitions of the direct path (resnet_ops.hip bn_parts)"""
    return max(1, min(1024, ((rows * C) >> 16) // ((C + 511) // 512)))


def measure_k_ref(device, shapes, log=print):
    """worst error / (2^-24 mag) per check of fp32_eval over `shapes` [(rows, C, dtype, affine)], both
    summation conventions"""
    worst = {}
    for i, (rows, C, dtype, affine) in enumerate(shapes):
        for pivot in (True, False):
            c = make_case(rows, C, dtype, device, 1000 + i, rows > 1, True, affine)
            rep = check_all(c, fp32_eval(c, pivot), pivot, measure=True)
            for n, v in rep.worst.items():
                n = n.split("[")[0]
                if n in K:
                    worst[n] = max(worst.get(n, 0.0), v)
            del c, rep
        log("k_ref after %d x %d %s: %s" % (rows, C, dtype, {n: round(v, 3) for n, v in worst.items()}))
    return worst
