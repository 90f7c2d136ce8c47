"""fp64 references of LayerNorm over rows, LayerNorm over whole maps and column sums, and the per-element /
per-column checks that pin the kernels of norm.hip and the `mapln_*` kernels of det_ops.hip to them
(tests/test_gpu_layernorm_kernels.py; proof that the checks bite: tests/test_ln_checks_cpu.py).

Reference, the textbook formulae in torch float64:
    mean = E_c[x], var = E_c[(x - mean)^2] (biased), rstd = (var + eps)^-1/2, xhat = (x - mean) rstd,
    y = xhat gamma + beta,
    g = gamma dy, dx = dres + rstd (g - E_c[g] - xhat E_c[g xhat]), dgamma = sum_r dy xhat, dbeta = sum_r dy
(`ref_row_forward`, `ref_row_backward`).  The map LayerNorm (`nn.LayerNorm((C, H, W))` on a channels-last map) is
the same with one row per image, M = H W C columns and a per-element affine in channels-last order, dw / db summed
over the images (`ref_map_forward`, `ref_map_backward`).  `ref_colsum`: out[c] = sum_r x[r, c] (+ initial).

What is compared with what (the convention of bn_checks).  The statistics a kernel returns are compared with the
fp64 statistics of x.  Every OTHER output is compared with the fp64 evaluation that starts from exactly what the
kernel was handed or returned in fp32: y from the (mean, rstd) the forward returned, the backward from the
(mean, rstd) it was given.  An error of the statistics is charged to the statistics checks and nothing else.

Bounds: |got - ref| <= u |ref| + k 2^-24 mag, per element or per column, never a global norm.
  u = 2^-8 for a bf16 output (one final rounding), 0 otherwise;
  mag = the fp64 sum of the ABSOLUTE values of the terms that are added:
    mean (row)      mean_c |x|                                      (the kernel sums about 0)
    rstd (row)      rstd^3 / 2 mean_c (x - mean)^2 + rstd           (two-pass about its own mean)
    y               |x a| + |mean a| + |beta|, a = rstd gamma
    dx              |dres| + rstd (|g| + mean_c |g| + |xhat| mean_c |g xhat|), g = gamma dy
    dgamma, dbeta   sum_r |dy xhat|, sum_r |dy|                     (+ |initial value| with accumulate)
    colsum          sum_r |x|                                       (+ |initial value|)
    map_mean        mean_i |x - mean|      about the MEAN, not about a pivot; plus 2^-24 |mean| outside the factor
                    k: the result is itself rounded to fp32 at its own size, whatever the spread of x is
    map_var         mean_i (x - mean)^2    (only an emulation returns it; the kernels return rstd)
    map_rstd        rstd^3 / 2 mean_i (x - mean)^2 + rstd
    map_y, map_dx, map_dw, map_db: as y, dx, dgamma, dbeta with the per-element w / bias and sums over the images
  dx_lp must be dx rounded to the operand type, bit for bit (both are stored from one register value; fp32: equal);
  y of a save_stats=False call must be the save_stats=True result, bit for bit; with integer dy, dbeta and colsum
  are exact (`exact=True`: torch.equal).

k.  Procedure (as in bn_checks / attn_checks): evaluate the same formulae in plain fp32 torch (`fp32_eval`,
`fp32_eval_map`, `fp32_colsum`: two-pass statistics for the row AND the map LayerNorm, `sum()` reductions;
neither the kernels nor the engine), run it through these checks over the case list of the GPU module
(`measure_k_ref`), record the worst error / (2^-24 mag) per check as k_ref, and set
k = max(16, 4 k_ref) rounded up to a power of two; k_ref is the larger of torch on the CPU and torch on the
MI355X.  The case list is `gpu_row_specs`, `gpu_fwd_only_specs`, `gpu_map_specs`, `gpu_colsum_specs` below, which is
what tests/test_gpu_layernorm_kernels.py runs; the CPU figures leave out the production rows and the pyramid maps.
NOT YET MEASURED on an MI355X: the k_ref (MI355X) column and the kernels' own worst ratios are empty, K_REF_GPU is
empty and k rests on the CPU column alone — `measure_k_ref("cuda")` fills the first, the last test of the GPU module
prints the second.  map_mean: the reference's 19.2 is the `offset` family (a mean of 30 sigma summed about 0 in
fp32: an error of |mean|, bounded about the mean); every other family stays below 2.2.

    check      k_ref CPU  k_ref MI355X  k     kernels' worst ratio
    mean           3.07            -    16     -
    rstd           2.14            -    16     -
    y              3.19            -    16     -
    dx             3.23            -    16     -
    dgamma         2.81            -    16     -
    dbeta          1.94            -    16     -
    colsum         1.08            -    16     -
    map_mean      19.16            -   128     -
    map_var        4.15            -    32     -
    map_rstd       2.06            -    16     -
    map_y          3.43            -    16     -
    map_dx         3.09            -    16     -
    map_dw         4.24            -    32     -
    map_db         2.83            -    16     -

Input families (all generated on the CPU from fixed seeds, `row_case` / `map_case`):
    gauss      per-row scale in [0.5, 2], per-row mean ~ N(0, 1)
    offset     a per-row mean of +-30 sigma (residual-stream drift)
    massive    two columns (map: two channels) at 100 times the rest
    tiny       scale 1e-4: var comparable with eps
    const      every row (image) constant, a multiple of 1/4 in [-8, 8] (every partial sum is exact in fp32, in any
               order: the mean is exact, var = 0 and rstd = eps^-1/2 — an fp32 mean that is off by e turns into
               var = e^2, which eps = 1e-6 does not hide for |x| ~ 8; that is the formula's, not a kernel's, doing)
    integers   integer x and dy: dbeta / db and colsum are exact
    outlier_first_K / outlier_elsewhere_K (map only, K = 50, 500): N(3, 1) with ONE element K sigma out, at
               element 0 (the pivot of a sum about the image's first element) / at element 1
  gamma ~ N(0, 1) with gamma[0] = 0 and gamma[1] < 0; beta ~ 0.3 N(0, 1).
"""
import math

import torch

EPS32 = 2.0 ** -24
F64 = torch.float64
F32, BF = torch.float32, torch.bfloat16
ROW_CHECKS = ("mean", "rstd", "y", "dx", "dgamma", "dbeta")
MAP_CHECKS = ("map_mean", "map_var", "map_rstd", "map_y", "map_dx", "map_dw", "map_db")
CHECKS = ROW_CHECKS + ("colsum",) + MAP_CHECKS
# worst error / (2^-24 mag) of the fp32 torch evaluation over the case list (measure_k_ref): torch on the CPU and
# torch on the MI355X, and the larger of the two
K_REF_CPU = {"mean": 3.070, "rstd": 2.141, "y": 3.188, "dx": 3.231, "dgamma": 2.811, "dbeta": 1.935,
             "colsum": 1.080, "map_mean": 19.165, "map_var": 4.151, "map_rstd": 2.061,
             "map_y": 3.431, "map_dx": 3.093, "map_dw": 4.243, "map_db": 2.828}
K_REF_GPU = {}
K_REF = {n: max(K_REF_CPU.get(n, 0.0), K_REF_GPU.get(n, 0.0)) for n in CHECKS}


def k_from(k_ref):
    return max(16, 2 ** math.ceil(math.log2(max(4.0 * k_ref, 1.0))))


K = {name: k_from(v) for name, v in K_REF.items()}


def u_of(dtype):
    return 2.0 ** -8 if dtype == torch.bfloat16 else 0.0


class Report:
    """worst error / (2^-24 mag) per check, and the checks that exceeded their k"""

    def __init__(self, k=None, tag="", measure=False):
        self.k = K if k is None else k
        self.tag = tag
        self.measure = measure      # record the ratios, fail none (k_ref)
        self.worst = {}
        self.failed = []

    def ratio(self, name, got, ref, mag, u=0.0, slack=0.0, kname=None):
        k = self.k[kname or name]
        got = got.to(F64)
        ref = ref.reshape(got.shape)
        err = ((got - ref).abs() - u * ref.abs() - slack).clamp_min(0)
        r = err / (EPS32 * mag)
        r = torch.where(err == 0, torch.zeros_like(r), r)           # 0 / 0: an exact value
        r = torch.nan_to_num(r, nan=math.inf, posinf=math.inf).reshape(-1)
        m, i = r.max(0)
        m, i = float(m), int(i)
        self.worst[name] = max(self.worst.get(name, 0.0), m)
        if not m <= k and not self.measure:
            self.failed.append("%s %s: error = %.4g x 2^-24 mag > k = %g at flat index %d of shape %s: got %.9g, ref %.9g"
                               % (self.tag, name, m, k, i, tuple(got.shape), float(got.reshape(-1)[i]),
                                  float(ref.reshape(-1)[i])))

    def same(self, name, got, want, what):
        """bit-for-bit"""
        if self.measure:
            return
        if got.dtype != want.dtype or not torch.equal(got, want):
            bad = (got.float() != want.float()).reshape(-1)
            i = int(bad.nonzero()[0]) if bool(bad.any()) else -1
            self.worst[name] = math.inf
            self.failed.append("%s %s: %s at %d elements, first at flat index %d: got %.9g, want %.9g"
                               % (self.tag, name, what, int(bad.sum()), i, float(got.reshape(-1)[i]),
                                  float(want.reshape(-1)[i])))

    def names(self):
        return sorted({f.split(":")[0].split()[-1] for f in self.failed})

    def merge(self, other):
        for n, v in other.worst.items():
            self.worst[n] = max(self.worst.get(n, 0.0), v)
        self.failed += other.failed
        return self

    def assert_ok(self):
        assert not self.failed, "\n".join(self.failed)


# ------------------------------------------------------------------ fp64 reference
def _stats(x, eps):
    xd = x.to(F64)
    mean = xd.mean(-1, keepdim=True)
    d = xd - mean
    var = (d * d).mean(-1, keepdim=True)
    return xd, mean, d, var, (var + eps) ** -0.5


def ref_row_forward(x, gamma, beta, eps, mean=None, rstd=None):
    """fp64 statistics of x over its last axis with the mags of their bounds, and y evaluated from the given
    (mean, rstd) [rows] (None: from the fp64 ones) with its mag"""
    xd, m, d, var, r = _stats(x, eps)
    o = {"mean": m[..., 0], "var": var[..., 0], "rstd": r[..., 0],
         "t_mean": xd.abs().mean(-1), "t_mean_c": d.abs().mean(-1), "t_var": var[..., 0],
         "t_rstd": (0.5 * r ** 3 * var + r)[..., 0]}
    del d
    mu = m if mean is None else mean.to(F64).reshape(m.shape)
    a = (r if rstd is None else rstd.to(F64).reshape(m.shape)) * gamma.to(F64)
    b = beta.to(F64)
    o["y"] = (xd - mu) * a + b
    o["t_y"] = (xd * a).abs() + (mu * a).abs() + b.abs()
    return o


def ref_row_backward(dy, x, gamma, mean, rstd, dres=None, dg0=None, db0=None):
    """fp64 backward from the handed (mean, rstd); dg0 / db0: what dgamma / dbeta held before an accumulating call"""
    xd, dyd = x.to(F64), dy.to(F64)
    cols = x.shape[-1]
    mu, rs = mean.to(F64).reshape(-1, 1), rstd.to(F64).reshape(-1, 1)
    xd, dyd = xd.reshape(-1, cols), dyd.reshape(-1, cols)
    xhat = (xd - mu) * rs
    g = dyd * gamma.to(F64)
    gx = g * xhat
    dx = rs * (g - g.mean(-1, keepdim=True) - xhat * gx.mean(-1, keepdim=True))
    t_dx = rs * (g.abs() + g.abs().mean(-1, keepdim=True) + xhat.abs() * gx.abs().mean(-1, keepdim=True))
    del g, gx
    if dres is not None:
        dx = dx + dres.to(F64).reshape(-1, cols)
        t_dx = t_dx + dres.to(F64).reshape(-1, cols).abs()
    dyx = dyd * xhat
    o = {"dx": dx, "t_dx": t_dx, "dgamma": dyx.sum(0), "t_dgamma": dyx.abs().sum(0),
         "dbeta": dyd.sum(0), "t_dbeta": dyd.abs().sum(0)}
    if dg0 is not None:
        o["dgamma"], o["t_dgamma"] = o["dgamma"] + dg0.to(F64), o["t_dgamma"] + dg0.to(F64).abs()
    if db0 is not None:
        o["dbeta"], o["t_dbeta"] = o["dbeta"] + db0.to(F64), o["t_dbeta"] + db0.to(F64).abs()
    return o


def ref_map_forward(x, w, bias, eps, mean=None, rstd=None):
    """x [B, ...] with M elements per image, w / bias [M] in x's element order"""
    B = x.shape[0]
    return ref_row_forward(x.reshape(B, -1), w.reshape(-1), bias.reshape(-1), eps, mean, rstd)


def ref_map_backward(dy, x, w, mean, rstd, dw0=None, db0=None):
    B = x.shape[0]
    return ref_row_backward(dy.reshape(B, -1), x.reshape(B, -1), w.reshape(-1), mean, rstd, None,
                            None if dw0 is None else dw0.reshape(-1), None if db0 is None else db0.reshape(-1))


def ref_colsum(x, init=None):
    """fp64 column sums of x [rows, cols] (+ init) and the mag of their bound"""
    xd = x.to(F64)
    s, t = xd.sum(0), xd.abs().sum(0)
    if init is not None:
        s, t = s + init.to(F64), t + init.to(F64).abs()
    return s, t


# ------------------------------------------------------------------ checks
def check_row_forward(rep, x, gamma, beta, eps, y, mean, rstd, pre=""):
    """mean / rstd [rows] against the statistics of x; y against the evaluation from (mean, rstd).  pre = "map_":
    the map LayerNorm's names and its statistics' mags (about the mean)"""
    fw = ref_row_forward(x, gamma, beta, eps, mean, rstd)
    if pre:
        rep.ratio(pre + "mean", mean, fw["mean"], fw["t_mean_c"], slack=EPS32 * fw["mean"].abs())
    else:
        rep.ratio("mean", mean, fw["mean"], fw["t_mean"])
    rep.ratio(pre + "rstd", rstd, fw["rstd"], fw["t_rstd"])
    if y is not None:
        rep.ratio(pre + "y", y.reshape(fw["y"].shape), fw["y"], fw["t_y"], u_of(y.dtype))
    return fw


def round_to(dx, dtype):
    return dx.to(dtype)       # torch rounds to nearest even, as the kernels' packing does


def check_row_backward(rep, dy, x, gamma, mean, rstd, dres, dx, dx_lp=None, dgamma=None, dbeta=None, dg0=None,
                       db0=None, exact=False, pre=""):
    bw = ref_row_backward(dy, x, gamma, mean, rstd, dres, dg0, db0)
    n = (lambda s: pre + {"dgamma": "dw", "dbeta": "db"}.get(s, s)) if pre else (lambda s: s)
    rep.ratio(n("dx"), dx.reshape(bw["dx"].shape), bw["dx"], bw["t_dx"], u_of(dx.dtype))
    if dx_lp is not None:
        rep.same("dx_lp", dx_lp, round_to(dx, dx_lp.dtype), "not dx rounded to the operand type")
    if dgamma is not None:
        rep.ratio(n("dgamma"), dgamma.reshape(-1), bw["dgamma"], bw["t_dgamma"])
    if dbeta is not None:
        rep.ratio(n("dbeta"), dbeta.reshape(-1), bw["dbeta"], bw["t_dbeta"])
        if exact:
            rep.same(n("dbeta"), dbeta.reshape(-1).to(F64), bw["dbeta"], "not the exact integer sum")
    return bw


def check_colsum(rep, x, out, init=None, exact=False, name="colsum"):
    s, t = ref_colsum(x, init)
    rep.ratio(name, out, s, t, kname="colsum")
    if exact:
        rep.same(name, out.to(F64), s, "not the exact integer sum")


# ------------------------------------------------------------------ cases
ROW_FAMILIES = ("gauss", "offset", "massive", "tiny", "const", "integers")
MAP_FAMILIES = ROW_FAMILIES + ("outlier_first_50", "outlier_first_500", "outlier_elsewhere_50", "outlier_elsewhere_500")
ROW_EPS, MAP_EPS = 1e-6, 1e-5


def _gen(seed):
    return torch.Generator("cpu").manual_seed(seed)


def _family_x(family, rows, cols, g, chan=None):
    rn = lambda *s: torch.randn(*s, generator=g)
    if family == "gauss":
        return rn(rows, cols) * (0.5 + 1.5 * torch.rand(rows, 1, generator=g)) + rn(rows, 1)
    if family == "offset":
        sign = 1.0 - 2.0 * (torch.arange(rows) % 2).float().view(rows, 1)
        return rn(rows, cols) + 30.0 * sign
    if family == "massive":
        x = rn(rows, cols)
        if chan is None:
            x[:, 1] *= 100.0
            x[:, cols - 2] *= 100.0
        else:           # channels 1 and chan - 2 of a channels-last map
            x.view(rows, -1, chan)[:, :, 1] *= 100.0
            x.view(rows, -1, chan)[:, :, chan - 2] *= 100.0
        return x
    if family == "tiny":
        return 1e-4 * rn(rows, cols)
    if family == "const":
        return (torch.randint(-32, 33, (rows, 1), generator=g).float() / 4).expand(rows, cols).contiguous()
    if family == "integers":
        return torch.randint(-4, 5, (rows, cols), generator=g).float()
    kind, sigmas = family.rsplit("_", 1)
    x = rn(rows, cols) + 3.0
    x[:, 0 if kind == "outlier_first" else 1] = 3.0 + float(sigmas)
    return x


def _affine(cols, g):
    gamma, beta = torch.randn(cols, generator=g), 0.3 * torch.randn(cols, generator=g)
    gamma[0] = 0.0
    gamma[1] = -gamma[1].abs() - 0.1
    return gamma, beta


def row_case(family, rows, cols, y_dtype=F32, dy_dtype=F32, dres=True, accumulate=False, seed=0):
    """a row LayerNorm case, generated on the CPU (the same on every machine)"""
    g = _gen(1 + seed + 7919 * cols + 104729 * rows + 31 * ROW_FAMILIES.index(family))
    gamma, beta = _affine(cols, g)
    dy = torch.randint(-3, 4, (rows, cols), generator=g).float() if family == "integers" \
        else torch.randn(rows, cols, generator=g)
    return {"family": family, "rows": rows, "cols": cols, "eps": ROW_EPS, "y_dtype": y_dtype, "dy_dtype": dy_dtype,
            "x": _family_x(family, rows, cols, g), "gamma": gamma, "beta": beta, "dy": dy.to(dy_dtype),
            "dres": torch.randn(rows, cols, generator=g) if dres else None,
            "dg0": torch.randn(cols, generator=g) if accumulate else None,
            "db0": torch.randn(cols, generator=g) if accumulate else None}


def map_case(family, B, M, dtype=F32, chan=8, accumulate=False, seed=0):
    """a map LayerNorm case: x, dy [B, M] in `dtype` (M = H W chan, channels-last), w / bias fp32 [M]"""
    g = _gen(3 + seed + 7919 * (M % 1000003) + 104729 * B + 31 * MAP_FAMILIES.index(family))
    w, bias = _affine(M, g)
    dy = torch.randint(-3, 4, (B, M), generator=g).float() if family == "integers" else torch.randn(B, M, generator=g)
    return {"family": family, "B": B, "M": M, "chan": chan, "eps": MAP_EPS, "dtype": dtype,
            "x": _family_x(family, B, M, g, chan).to(dtype), "w": w, "bias": bias, "dy": dy.to(dtype),
            "dw0": torch.randn(M, generator=g) if accumulate else None,
            "db0": torch.randn(M, generator=g) if accumulate else None}


def colsum_case(family, rows, cols, ld, dtype=F32, accumulate=False, seed=0):
    """x: a [rows, cols] window (a view with row stride ld) of a wider matrix"""
    g = _gen(5 + seed + 7919 * cols + 104729 * rows + ld)
    wide = (torch.randint(-3, 4, (rows, ld), generator=g).float() if family == "integers"
            else torch.randn(rows, ld, generator=g)).to(dtype)
    return {"family": family, "rows": rows, "cols": cols, "ld": ld, "dtype": dtype, "wide": wide,
            "x": wide[:, :cols], "init": torch.randn(cols, generator=g) if accumulate else None}


def to_device(c, device):
    return {k: v.to(device) if torch.is_tensor(v) else v for k, v in c.items()}


# ------------------------------------------------------------------ the same formulae in plain fp32 torch
# name -> (what it is applied to, a check that must fail)
MUTATIONS = {
    "unbiased_var": ("row", "rstd"),
    "eps_outside_sqrt": ("row", "rstd"),
    "mean_over_padded_cols": ("row", "mean"),
    "last_strip_dropped": ("row", "y"),
    "bwd_rows_ge_4096_skipped": ("row", "dx"),
    "wave3_rows_missing": ("row", "dbeta"),
    "last_partial_row_dropped": ("row", "dbeta"),
    "dgamma_dbeta_exchanged": ("row", "dgamma"),
    "split_off_by_a_strip": ("row", "dbeta"),
    "dgamma_from_x_rstd": ("row", "dgamma"),
    "dx_without_mean_g": ("row", "dx"),
    "dx_without_xhat_term": ("row", "dx"),
    "dx_gamma_not_applied": ("row", "dx"),
    "dres_dropped": ("row", "dx"),
    "dres_twice": ("row", "dx"),
    "rstd_of_neighbour_row": ("row", "y"),
    "beta_dropped": ("row", "y"),
    "accumulate_ignored": ("row", "dgamma"),
    "dx_lp_truncated": ("row", "dx_lp"),
    "map_pivot_without_d2": ("map", "map_rstd"),
    "map_affine_nchw": ("map", "map_y"),
    "map_bwd_means_exchanged": ("map", "map_dx"),
    "map_dw_first_image_only": ("map", "map_dw"),
    "colsum_ld_as_cols": ("colsum", "colsum"),
}


def ln_bwd_blocks(rows):
    return min((rows + 3) // 4, 1024)       # norm.hip: 4 rows (waves) per block, at most 1024 blocks


def _truncate_bf16(t):
    return (t.contiguous().view(torch.int32) & -65536).view(torch.float32).to(BF)


def fp32_eval(c, mut=None, dt=F32):
    """row LayerNorm forward + backward of case `c` in `dt`: two-pass statistics, sum() reductions.
    `mut`: one of MUTATIONS — a deliberately wrong variant (tests/test_ln_checks_cpu.py)"""
    x, rows, cols, eps = c["x"].to(dt), c["rows"], c["cols"], c["eps"]
    gamma, beta = c["gamma"].to(dt), c["beta"].to(dt)
    n = 256 * ((cols + 255) // 256) if mut == "mean_over_padded_cols" else cols
    mean = x.sum(-1, keepdim=True) / n
    d = x - mean
    var = (d * d).sum(-1, keepdim=True) / (cols - 1 if mut == "unbiased_var" and cols > 1 else cols)
    rstd = 1.0 / (var.sqrt() + eps) if mut == "eps_outside_sqrt" else torch.rsqrt(var + eps)
    rs_y = rstd.roll(1, 0) if mut == "rstd_of_neighbour_row" else rstd
    y = (x - mean) * rs_y * gamma + (0.0 if mut == "beta_dropped" else beta)
    dy = c["dy"].to(dt)
    xhat = (x - mean) * rstd
    g = gamma * dy
    s1 = 0.0 if mut == "dx_without_mean_g" else g.sum(-1, keepdim=True) / cols
    s2 = 0.0 if mut == "dx_without_xhat_term" else (g * xhat).sum(-1, keepdim=True) / cols
    dx = rstd * ((dy if mut == "dx_gamma_not_applied" else g) - s1 - xhat * s2)
    if c["dres"] is not None and mut != "dres_dropped":
        dx = dx + c["dres"].to(dt) * (2.0 if mut == "dres_twice" else 1.0)
    r = torch.arange(rows, device=x.device)
    keep = torch.ones(rows, dtype=torch.bool, device=x.device)
    if mut == "bwd_rows_ge_4096_skipped":
        keep = r < 4096
        dx = torch.where(keep.view(-1, 1), dx, torch.zeros_like(dx))
    elif mut == "wave3_rows_missing":
        keep = r % 4 != 3
    elif mut == "last_partial_row_dropped":
        nb = ln_bwd_blocks(rows)
        keep = (r // 4) % nb != nb - 1
    kd = dy[keep]
    dgamma = (kd * (x * rstd if mut == "dgamma_from_x_rstd" else xhat)[keep]).sum(0)
    dbeta = kd.sum(0)
    dg0 = torch.zeros(cols, dtype=dt, device=x.device) if c["dg0"] is None else c["dg0"].to(dt)
    db0 = torch.zeros(cols, dtype=dt, device=x.device) if c["db0"] is None else c["db0"].to(dt)
    if mut == "split_off_by_a_strip" and cols >= 128:      # [dgamma | dbeta] cut 64 columns early
        both = torch.cat([dgamma, dbeta])
        dgamma = torch.cat([both[:cols - 64], torch.zeros(64, dtype=dt, device=x.device)])
        dbeta = both[cols - 64:2 * cols - 64]
    if mut == "dgamma_dbeta_exchanged":
        dgamma, dbeta = dbeta, dgamma
    if mut != "accumulate_ignored":
        dgamma, dbeta = dgamma + dg0, dbeta + db0
    o = {"mean": mean[:, 0], "rstd": rstd[:, 0], "y": y.to(c["y_dtype"]), "dx": dx.float(), "dgamma": dgamma,
         "dbeta": dbeta}
    o["dx_lp"] = _truncate_bf16(o["dx"]) if mut == "dx_lp_truncated" and c["dy_dtype"] == BF \
        else o["dx"].to(c["dy_dtype"])
    if mut == "last_strip_dropped":
        for name in ("y", "dx", "dx_lp"):
            o[name][:, -4:] = 0
    return o


def check_row_all(c, o, k=None, tag="", measure=False):
    """every row check on the outputs `o` (keys as fp32_eval returns them) of case `c`"""
    rep = Report(k, tag or "%s %dx%d" % (c["family"], c["rows"], c["cols"]), measure)
    check_row_forward(rep, c["x"], c["gamma"], c["beta"], c["eps"], o["y"], o["mean"], o["rstd"])
    check_row_backward(rep, c["dy"], c["x"], c["gamma"], o["mean"], o["rstd"], c["dres"], o["dx"], o.get("dx_lp"),
                       o["dgamma"], o["dbeta"], c["dg0"], c["db0"], exact=c["family"] == "integers" and c["db0"] is None)
    return rep


def map_stats_by_parts(x, V, nparts=256, dt=F32):
    """(mean, var) [B, 1] of x [B, M] the way det_ops.hip takes them: part p owns the V-element vectors
    p * 256 + t + k * 256 * nparts, sums them about 0 for a first mean m0, then d = x - m0 and d^2 for its
    (mean, M2); the (count, mean, M2) triples are combined about the mean of the part means"""
    B, M = x.shape
    K = -(-M // (256 * nparts * V))
    lay = lambda t: torch.nn.functional.pad(t, (0, K * 256 * nparts * V - M)).view(B, K, nparts, 256 * V) \
        .transpose(1, 2).reshape(B, nparts, -1)
    xp, inside = lay(x.to(dt)), lay(torch.ones(B, M, dtype=dt, device=x.device))
    n = inside[0].sum(-1)
    used = n > 0
    nz = n.clamp_min(1)
    m0 = xp.sum(-1) / nz
    d = (xp - m0[:, :, None]) * inside
    s, q = d.sum(-1), (d * d).sum(-1)
    mp = m0 + s / nz
    m2 = (q - s * (s / nz)).clamp_min(0)
    g0 = (n * mp).sum(-1, keepdim=True) / M
    mean = g0 + (n * (mp - g0)).sum(-1, keepdim=True) / M
    var = (torch.where(used, m2 + n * (mp - mean) ** 2, torch.zeros_like(m2))).sum(-1, keepdim=True) / M
    return mean, var


def fp32_eval_map(c, mut=None, pivot=False, parts=False, dt=F32):
    """map LayerNorm of case `c` in `dt`; pivot=True: the statistics as sums about the image's first element,
    var = E[d^2] - E[d]^2 (the one-pass formula), instead of two passes; parts=True: as the kernels take them"""
    x, B, M, eps = c["x"].to(dt), c["B"], c["M"], c["eps"]
    w, bias = c["w"].to(dt), c["bias"].to(dt)
    if mut == "map_affine_nchw":        # [H W, chan] read as [chan, H W]
        w, bias = (t.view(-1, c["chan"]).t().reshape(-1) for t in (w, bias))
    if parts:
        mean, var = map_stats_by_parts(x, 8 if c["dtype"] == BF else 4)
    elif pivot or mut == "map_pivot_without_d2":
        piv = x[:, :1]
        d = x - piv
        dm = d.sum(-1, keepdim=True) / M
        var = (d * d).sum(-1, keepdim=True) / M
        if mut != "map_pivot_without_d2":
            var = var - dm * dm
        var = var.clamp_min(0)
        mean = piv + dm
    else:
        mean = x.sum(-1, keepdim=True) / M
        d = x - mean
        var = (d * d).sum(-1, keepdim=True) / M
    rstd = torch.rsqrt(var + eps)
    y = (x - mean) * rstd * w + bias
    dy = c["dy"].to(dt)
    xhat = (x - mean) * rstd
    g = w * dy
    m1, m2 = g.sum(-1, keepdim=True) / M, (g * xhat).sum(-1, keepdim=True) / M
    if mut == "map_bwd_means_exchanged":
        m1, m2 = m2, m1
    dx = rstd * (g - m1 - xhat * m2)
    nb = 1 if mut == "map_dw_first_image_only" else B
    dw, db = (dy * xhat)[:nb].sum(0), dy.sum(0)
    if c["dw0"] is not None:
        dw, db = dw + c["dw0"].to(dt), db + c["db0"].to(dt)
    return {"mean": mean[:, 0], "var": var[:, 0], "rstd": rstd[:, 0], "y": y.to(c["dtype"]), "dx": dx.to(c["dtype"]),
            "dw": dw, "db": db}


def check_map_all(c, o, k=None, tag="", measure=False):
    rep = Report(k, tag or "map %s %dx%d" % (c["family"], c["B"], c["M"]), measure)
    fw = check_row_forward(rep, c["x"], c["w"], c["bias"], c["eps"], o["y"], o["mean"], o["rstd"], pre="map_")
    if o.get("var") is not None:
        rep.ratio("map_var", o["var"], fw["var"], fw["t_var"])
    check_row_backward(rep, c["dy"], c["x"], c["w"], o["mean"], o["rstd"], None, o["dx"], None, o.get("dw"), o.get("db"),
                       c["dw0"], c["db0"], exact=c["family"] == "integers" and c["db0"] is None, pre="map_")
    return rep


def fp32_colsum(c, mut=None, dt=F32):
    x = c["x"]
    if mut == "colsum_ld_as_cols":      # the window read as if its rows were cols apart
        x = c["wide"].reshape(-1)[:c["rows"] * c["cols"]].view(c["rows"], c["cols"])
    s = x.to(dt).sum(0)
    return s if c["init"] is None else s + c["init"].to(dt)


def check_colsum_all(c, out, k=None, tag="", measure=False):
    rep = Report(k, tag or "colsum %s %dx%d ld %d" % (c["family"], c["rows"], c["cols"], c["ld"]), measure)
    check_colsum(rep, c["x"], out, c["init"], exact=c["family"] == "integers" and c["init"] is None)
    return rep


# ------------------------------------------------------------------ the case list of the GPU module
FWD_BWD_COLS = (4, 8, 64, 128, 192, 252, 256, 260, 384, 512, 516, 768, 1020, 1024)
FWD_ONLY_COLS = (1028, 1280, 1536, 2048)
MODEST_ROWS = 37        # nine full blocks and a partial one
# rows at every boundary of the launch geometry (cols 384 and 768): a partial block; the grid-stride loop (1024
# blocks of 4 rows); nparts = 15 .. 1024 of reduce_partials_kernel (rows = 4 nparts - 1: the last block partial)
GEOMETRY_COLS = (384, 768)
REDUCE_NPARTS = (15, 16, 17, 48, 49, 50, 240, 241, 242, 496, 497, 1024)
GEOMETRY_ROWS = (1, 2, 3, 4, 5, 4095, 4096, 4097) + tuple(4 * n - 1 for n in REDUCE_NPARTS if n < 1024)
PRODUCTION_ROWS = ((12800, 768), (12608, 768), (50432, 512), (12608, 384), (12608, 1024))
MAP_STRIDE = 256 * 256 * 8          # elements one pass of mapln's reduce loop covers in bf16 (fp32: half)
MAP_M = (8, 2880, MAP_STRIDE - 8, MAP_STRIDE + 8, 3 * MAP_STRIDE)
PYRAMID_MAPS = ((32, 32, 256), (64, 64, 256), (128, 128, 256), (128, 128, 768), (256, 256, 256))   # H, W, C
# (rows, cols): vector (cols % 4 == 0), narrow (cols / 4 a power of two <= 32) and scalar kernels; row counts
# around the 256-part (64 rows each) and the narrow kernel's 2048-part caps
COLSUM_SHAPES = ((1577, 2304), (1577, 384), (333, 6), (37, 130), (70001, 128), (2049, 64), (5, 8), (1, 4),
                 (16383, 260), (16384, 260), (16385, 260), (16449, 12),
                 (131071, 32), (131072, 32), (131137, 32))


def row_configs():
    """(y dtype, dy / dx_lp dtype, dres given, dx_lp wanted, accumulate)"""
    for i, (dyt, dres, lp) in enumerate((a, b, c) for a in (F32, BF) for b in (True, False) for c in (True, False)):
        yield (BF if i % 2 else F32), dyt, dres, lp, i % 3 == 0


def gpu_row_specs(production=True):
    """every backward-capable row case of the GPU module: (group, arguments of row_case, dx_lp wanted)"""
    for cols in FWD_BWD_COLS:
        for family in ROW_FAMILIES:
            for yt, dyt, dres, lp, acc in row_configs():
                yield "cols%d" % cols, (family, MODEST_ROWS, cols, yt, dyt, dres, acc), lp
    for cols in GEOMETRY_COLS:
        for rows in GEOMETRY_ROWS:
            yield "geometry%d" % cols, ("gauss", rows, cols, BF, BF, True, False), True
            yield "geometry%d" % cols, ("integers", rows, cols, F32, F32, False, False), False
    if production:
        for rows, cols in PRODUCTION_ROWS:
            yield "production%dx%d" % (rows, cols), ("gauss", rows, cols, BF, BF, True, False), True
            yield "production%dx%d" % (rows, cols), ("offset", rows, cols, BF, BF, True, True), True


def gpu_fwd_only_specs():
    for cols in FWD_ONLY_COLS:
        for family in ROW_FAMILIES:
            for yt in (F32, BF):
                yield "cols%d" % cols, (family, MODEST_ROWS, cols, yt, F32, False, False)


def gpu_map_specs(pyramid=True):
    """(group, arguments of map_case)"""
    for M in MAP_M:
        for B in (1, 3):
            for dtype in (F32, BF):
                fams = MAP_FAMILIES if M <= MAP_STRIDE + 8 or B == 1 else ("gauss", "outlier_first_500")
                for i, family in enumerate(fams):
                    yield "M%d-B%d-%s" % (M, B, "bf16" if dtype == BF else "fp32"), (family, B, M, dtype, 8, i % 2 == 1)
    if pyramid:
        for H, W, C in PYRAMID_MAPS:
            for family in ("gauss", "massive", "outlier_first_500"):
                yield "pyramid%dx%dx%d" % (H, W, C), (family, 1, H * W * C, BF, C, False)


def gpu_colsum_specs():
    """(group, arguments of colsum_case): ld = cols overwritten, and a window of a wider matrix accumulated"""
    for rows, cols in COLSUM_SHAPES:
        for dtype in (F32, BF):
            for family in ("gauss", "integers"):
                yield "%dx%d" % (rows, cols), (family, rows, cols, cols, dtype, False)
            yield "%dx%d" % (rows, cols), ("gauss", rows, cols, cols + 24, dtype, True)


def groups(specs):
    return list(dict.fromkeys(s[0] for s in specs))


def measure_k_ref(device, production=True, log=print):
    """worst error / (2^-24 mag) per check of the fp32 torch evaluation over the GPU module's case list"""
    worst = {}

    def note(rep, what):
        for n, v in rep.worst.items():
            if v > worst.get(n, 0.0):
                worst[n] = v
                log("k_ref %s = %.3f at %s" % (n, v, what))
    for grp, a, _ in gpu_row_specs(production):
        c = to_device(row_case(*a), device)
        note(check_row_all(c, fp32_eval(c), measure=True), grp + " " + a[0])
    for grp, a in gpu_fwd_only_specs():
        c = to_device(row_case(*a), device)
        o = fp32_eval(c)
        rep = Report(measure=True)
        check_row_forward(rep, c["x"], c["gamma"], c["beta"], c["eps"], o["y"], o["mean"], o["rstd"])
        note(rep, grp + " " + a[0])
    for grp, a in gpu_map_specs(production):
        c = to_device(map_case(*a), device)
        note(check_map_all(c, fp32_eval_map(c), measure=True), "map " + grp + " " + a[0])
    for grp, a in gpu_colsum_specs():
        c = to_device(colsum_case(*a), device)
        note(check_colsum_all(c, fp32_colsum(c), measure=True), "colsum " + grp)
    return worst
