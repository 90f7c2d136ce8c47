"""fp64 reference of the GEMM entry points (ssl4gie_gemm, ssl4gie_gemm_tn_pair, ssl4gie_gemm_tn_group) with every
epilogue of include/ssl4gie_hip.h, and the per-element checks that pin the kernels of gemm.hip, gemm_nt256.hip,
gemm_tn256.hip and gemm256.h to it (tests/test_gpu_gemm_kernels.py; proof that the checks bite:
tests/test_gemm_checks_cpu.py).  The implicit-convolution operand (`desc.conv`, EPI_RELU_MASK_AUX) belongs to
tests/test_gpu_conv.py and stays out.

Reference, plain torch float64 from the operands exactly as handed (bf16 values are exact in fp64):
    acc = sum_k A(m,k) B(k,n), mag_acc = sum_k |A(m,k)| |B(k,n)|, then the epilogue in fp64 (`reference`):
    0 NONE            alpha acc (+ C_initial with accumulate)
    1 BIAS            alpha acc + bias[n]
    2 BIAS_GELU       C = u = alpha acc + bias[n], out2 = gelu(u)
    3 BIAS_RESIDUAL   alpha acc + bias[n] + residual[m,n]
    4 DGELU           alpha acc gelu'(aux[m,n])
    5 BIAS_GELU_GRAD  C = gelu'(u), out2 = gelu(u)
    6 MUL_AUX         alpha acc aux[m,n]
    8 ADD_AUX         alpha acc + aux[m,n]
    9 AFFINE_AUX_RELU act(alpha acc scale[n] + bias[n] (+ aux[m,n])), act = ReLU if `relu`
    colsum_a[m] = sum_k A(m,k) (+ initial value with accumulate)
    colstats[r][0/1][n] = sums / sums of squares over rows 128 r .. 128 r + 127 < M of the bf16 C THE KERNEL RETURNED
    (judged from what was stored, as the header defines it); the statistics-only product (C == NULL) must equal the
    storing product's statistics bit for bit (the GPU module).

Bounds, per element, never a norm:  |got - ref| <= u |ref| + k 2^-24 mag + g
    u = 2^-8 for a bf16 output (one rounding), 0 for fp32;
    mag = the sum of the absolute values of the terms that are added:
        modes 0, 1, 3, 8    |alpha| mag_acc (+ |bias| + |residual| + |C_initial| + |aux|)
        MUL_AUX, DGELU      |alpha| mag_acc |factor| (factor = aux resp. the fp64 gelu'(aux))
        AFFINE              |alpha scale| mag_acc + |bias| + |aux|       (ReLU is 1-Lipschitz: the bound stands)
        colsum_a            sum_k |A| (+ |initial|);      colstats  sum |y|, sum y^2
    g is non-zero for the GELU outputs only.  The pre-activation u is returned rounded or not at all, so gelu(u) and
    gelu'(u) are judged from the fp64 u: with b_u = k 2^-24 mag_u the bound of u before its output rounding,
        gelu(u)   1.13 b_u + A_g(u)       (sup |gelu'|  = 1.13)
        gelu'(u)  0.80 b_u + A_d(u)       (sup |gelu''| = 0.80)
        DGELU     (|alpha acc| + b_acc) A_d(aux)   (the factor's own error times the product it multiplies)
    and A the approximation term of the form the route uses (GELU_FORMS):
        erf    gemm.hip gelu_f / dgelu_f (erff; generic kernel)        A_g = c_g |u| 2^-24,  A_d = c_d 2^-24
        poly   common.h gelu_parts_fast / gelu_grad4_fast (A&S 7.1.26) A_g = c_g |u| 2^-24,  A_d = c_d 2^-24
        table  gelu_table.h on the 256-wide bf16 tile (Phi, gelu' at the bf16-ROUNDED u): the bounds of
               tests/test_gpu_gelu_table.py::test_gelu_table_accuracy_cpu, imported from there (`bound_g`, and
               `DGELU_ABS` = 8e-3 absolute for gelu'); both already contain the output rounding, so u = 0 there.
    c_g, c_d are measured (`measure_gelu_constants`): the form restated in fp32 torch against the fp64 erf forms on a
    dense grid of u in [-20, 20] plus +-2^-12, +-16, +-30, +-1e4, the worst ratio times 4 (the device's __expf and rcp
    are each about 1 ulp worse than torch's) rounded up to a power of two:
        form   worst c_g  worst c_d   c_g  c_d
        erf       1.73       2.10       8   16
        poly      4.47       4.43      32   32
    The erf form has an entry too: 1 + erff(x / sqrt 2) is rounded at the size of 1 whatever x is, an absolute error
    of 2^-25 in Phi that is not small against gelu'(x) in the negative tail (gelu'(-5) = -7e-6), where EPI_DGELU
    multiplies by it; without the term the fp32 evaluation of the textbook formula fails at the tails.

k.  Procedure (as in bn_checks / attn_checks / ln_checks): an fp32 torch EMULATION that is neither the kernels nor
`ops` (`emulate`): products summed exactly per 32-wide K chunk (one MFMA), the chunks added one after the other into an
fp32 accumulator, split-K partials formed per split range [nkt s / splits, nkt (s + 1) / splits) of 64-wide K-tiles
and added in slab order, epilogues in fp32; the generic kernel (f32 MFMA 16x16x4) as a k-ordered fmaf chain.  It
is run through these checks over the case list of the GPU module (`measure_k_ref`), the worst error / (2^-24 mag) per
check and accumulation-length class is k_ref, and k = max(16, 4 k_ref) rounded up to a power of two; k_ref is the
larger of torch on the CPU and torch on the MI355X.  Classes by L = ceil(K / 32 / splits) + splits, the longest chain
of sequential adds (K + 1 on the generic kernel: its chain has one link per k), edges at 16, 128 and 1024
(`acc_class`); the splits come from `route`.  The CPU column leaves out
the cases whose reference runs on the device (more than 1e8 multiply-adds).

    check            k_ref CPU  k_ref MI355X    k   kernels' worst ratio
    acc_L16             4.33        4.33        32        8.83
    acc_L128           11.22       11.22        64       11.22
    acc_L1024          11.66       15.29        64       21.22
    acc_Lbig           31.48       31.48       128       60.43
    colsum              1.55        1.20        16        1.29
    colstats            3.25        2.66        16        2.79
k_ref is the `offset` family's everywhere (gauss stays below 5, cancel below 0.5): 448 / 4096 / 32768 on one chain give
4.3 / 11.7 / 31.5, 65536 over 256 slabs 15.3, the generic chain of K = 100 gives 11.2 (the kernel's bits: its worst
ratio is the emulation's).  On the long chains the MFMA kernels sit at about twice the emulation, which adds each
32-wide chunk as ONE exactly summed term where the matrix core rounds inside the chunk as well; no kernel exceeds
half its k, and no k was taken from a kernel's figure.  The GELU constants with torch on the MI355X: erf 1.84 / 2.17,
poly 4.53 / 4.59 — the same c_g, c_d.

Input families (fixed seeds, generated on the CPU; `make_case`):
    gauss     x ~ 0.5 N, w ~ K^-1/2 N, bias ~ 0.1 N
    offset    same-sign operands: |ref| ~ mag
    cancel    the second half of K repeats the first with w negated: acc = 0 in exact arithmetic, only the k term
              allows anything; a dropped or duplicated K-tile is an error of order mag
    massive   two K-columns of x at 100 times the rest
    integers  small asymmetric integer ranges (w in eighths), alpha in {1, 0.5, -2}, bias / residual / aux / scale
              multiples of 2^-k: every fp32 intermediate is exact, the output must equal the fp64 value rounded once to
              the output type BIT FOR BIT for every epilogue without a transcendental (`exact`)
    onehot    the rows of A are one-hot, C selects an entry of B: the accumulator is known exactly at any magnitude;
              B and the bias make u sweep [-12, 12] densely and hit +-0, +-2^-12, +-16, +-30, +-1e4 — pins the GELU /
              GELU' / DGELU / affine arithmetic itself, tails and table clamps included
    vectors: scale[0] < 0, scale[1] = 0; the aux of EPI_DGELU sweeps the same grid (tails) in every family but
    `integers`; relu on and off, aux present and absent.

Layout of every case (`Window`): every output (C, out2, colsum_a, colstats) is a window of a buffer filled with the
sentinel -768 (ldc > N, a multiple of 8, and 4 (mod 8) on every other fp32 case outside the 256-wide NT kernels,
which refuse such an ldc; two spare rows before and after) and the check `guard` fails if one
sentinel changed; every operand (A, B, bias, residual, aux, scale) is a window between NaN bands (lda > K, ldb > K,
multiples of 8; ldr != ldc): a result may depend on nothing outside its operands.

`route(spec, cus)` restates the dispatch of ssl4gie_gemm in the default environment.  It labels the cases and builds
the table of variants; the two things a bound takes from it are the split count (the class of k) and the GELU form,
both confirmed by the kernel trace recorded in the GPU module's docstring.
"""
import math
import os
import sys

import torch

EPS32 = 2.0 ** -24
F64 = torch.float64
F32, BF = torch.float32, torch.bfloat16
NONE, BIAS, BIAS_GELU, BIAS_RESIDUAL, DGELU, BIAS_GELU_GRAD, MUL_AUX, RELU_MASK_AUX, ADD_AUX, AFFINE = range(10)
EPI_NAMES = {NONE: "none", BIAS: "bias", BIAS_GELU: "bias_gelu", BIAS_RESIDUAL: "bias_residual", DGELU: "dgelu",
             BIAS_GELU_GRAD: "bias_gelu_grad", MUL_AUX: "mul_aux", ADD_AUX: "add_aux", AFFINE: "affine_aux_relu"}
SENTINEL = -768.0
FAMILIES = ("gauss", "offset", "cancel", "massive", "integers", "onehot")
CLASSES = ("acc_L16", "acc_L128", "acc_L1024", "acc_Lbig")
CHECKS = CLASSES + ("colsum", "colstats")
# worst error / (2^-24 mag) of the emulation over the GPU module's case list (measure_k_ref)
K_REF_CPU = {"acc_L16": 4.325, "acc_L128": 11.223, "acc_L1024": 11.659, "acc_Lbig": 31.477, "colsum": 1.554, "colstats": 3.249}
K_REF_GPU = {"acc_L16": 4.325, "acc_L128": 11.223, "acc_L1024": 15.290, "acc_Lbig": 31.477, "colsum": 1.203, "colstats": 2.662}
K_REF = {n: max(K_REF_CPU.get(n, 0.0), K_REF_GPU.get(n, 0.0)) for n in CHECKS}
# (c_g, c_d) of the GELU forms and the worst ratios they come from (measure_gelu_constants)
GELU_WORST = {"erf": (1.73, 2.10), "poly": (4.47, 4.43)}


def k_from(k_ref):
    return max(16, 2 ** math.ceil(math.log2(max(4.0 * k_ref, 1.0))))


def c_from(worst):
    return 2 ** math.ceil(math.log2(4.0 * worst))


K = {name: k_from(v) for name, v in K_REF.items()}
GELU_C = {form: (c_from(g), c_from(d)) for form, (g, d) in GELU_WORST.items()}


def u_of(dtype):
    return 2.0 ** -8 if dtype == BF else 0.0


def acc_class(Kdim, splits=1, generic=False):
    """the class of k: by the longest chain of sequential adds (the generic kernel's fmaf chain is K long)"""
    L = Kdim + 1 if generic else -(-Kdim // (32 * splits)) + splits
    return CLASSES[0] if L <= 16 else CLASSES[1] if L <= 128 else CLASSES[2] if L <= 1024 else CLASSES[3]


class Report:
    """worst error / (2^-24 mag) per check name, and the checks that exceeded their k"""

    def __init__(self, k=None, tag="", measure=False):
        self.k = K if k is None else k
        self.tag = tag
        self.measure = measure      # record the ratios, fail none (k_ref)
        self.worst = {}
        self.failed = []
        self.failed_names = set()

    def ratio(self, name, got, ref, mag, u=0.0, slack=0.0, kname=None, kscale=1.0):
        """error beyond u |ref| + slack, in units of 2^-24 mag kscale; recorded under kname"""
        kname = kname or name
        k = self.k[kname]
        got = got.to(F64)
        ref = ref.reshape(got.shape)
        if got.numel() == 0:
            return
        err = ((got - ref).abs() - u * ref.abs() - slack).clamp_min(0)
        r = err / (EPS32 * mag * kscale)
        r = torch.where(err == 0, torch.zeros_like(r), r)           # 0 / 0: an exact value
        r = torch.nan_to_num(r, nan=math.inf, posinf=math.inf).reshape(-1)
        m, i = r.max(0)
        m, i = float(m), int(i)
        self.worst[kname] = max(self.worst.get(kname, 0.0), m)
        if not m <= k and not self.measure:
            shape = tuple(got.shape)
            pos = tuple(int(v) for v in torch.unravel_index(torch.tensor(i), shape)) if shape else ()
            self.failed_names.add(name)
            self.failed.append("%s %s: error = %.4g x 2^-24 mag > k(%s) = %g at %s of %s: got %.9g, ref %.9g"
                               % (self.tag, name, m, kname, k, pos, shape, float(got.reshape(-1)[i]),
                                  float(ref.reshape(-1)[i])))

    def same(self, name, got, want, what):
        """bit for bit"""
        if self.measure:
            return
        if got.dtype != want.dtype or got.shape != want.shape or not torch.equal(got, want):
            bad = (got.double() != want.double()).reshape(-1)
            i = int(bad.nonzero()[0]) if bool(bad.any()) else -1
            pos = tuple(int(v) for v in torch.unravel_index(torch.tensor(max(i, 0)), tuple(got.shape)))
            self.failed_names.add(name)
            self.failed.append("%s %s: %s at %d elements, first at %s of %s: got %.9g, want %.9g"
                               % (self.tag, name, what, int(bad.sum()), pos, tuple(got.shape),
                                  float(got.reshape(-1)[i]), float(want.reshape(-1)[i])))

    def guard(self, name, buf, win):
        """every element of `buf` outside the window still holds the sentinel"""
        out = win.outside().to(buf.device)
        bad = (buf != SENTINEL) & out
        if bool(bad.any()):
            i = int(bad.nonzero()[0])
            rel = i - win.off
            self.failed_names.add("guard")
            self.failed.append("%s guard: %s wrote outside its window at %d places, first %d elements from its start "
                               "(row %d, column %d of the leading dimension %d): %.9g"
                               % (self.tag, name, int(bad.sum()), rel, rel // max(win.ld, 1), rel % max(win.ld, 1),
                                  win.ld, float(buf[i])))

    def names(self):
        return sorted(self.failed_names)

    def merge(self, other):
        for n, v in other.worst.items():
            self.worst[n] = max(self.worst.get(n, 0.0), v)
        self.failed += other.failed
        self.failed_names |= other.failed_names
        return self

    def assert_ok(self):
        assert not self.failed, "\n".join(self.failed[:40])


# ------------------------------------------------------------------ windows of guarded buffers
class Window:
    """a strided window (shape, element strides) of a flat buffer filled with `fill`: NaN around an operand, the
    sentinel around an output; `ld` is the stride the window's rows are apart (for messages)"""

    def __init__(self, shape, strides, dtype, fill, ld=0):
        self.shape, self.strides, self.ld = tuple(shape), tuple(strides), int(ld)
        span = 1 + sum((s - 1) * st for s, st in zip(self.shape, self.strides)) if all(s > 0 for s in shape) else 0
        self.off = 2 * self.ld + 64                      # two spare rows (and 16-byte alignment) in front
        self.buf = torch.full((self.off + span + 2 * self.ld + 320,), fill, dtype=dtype)

    def view(self, buf=None):
        return torch.as_strided(self.buf if buf is None else buf, self.shape, self.strides, self.off)

    def outside(self):
        m = torch.ones(self.buf.numel(), dtype=torch.bool)
        torch.as_strided(m, self.shape, self.strides, self.off).fill_(False)
        return m

    def set(self, t):
        self.view().copy_(t)
        return self


def _up8(v):
    return 8 * (-(-v // 8))


def ldc_of(s):
    """ldc > N: a multiple of 8, or 4 (mod 8) for the fp32 outputs flagged ldc4"""
    if s["ldc4"]:
        ld = 4 * (-(-s["N"] // 4)) + 4
        return ld if ld % 8 == 4 else ld + 4
    return _up8(s["N"]) + 8


# ------------------------------------------------------------------ cases
def spec(M, N, Kdim, layout="nt", ab=BF, c=BF, epi=NONE, alpha=1.0, acc=False, colsum=False, colstats=False,
         c_null=False, relu=False, aux=True, bias=True, batch=(1, 1), family="gauss", cus=240, seed=0, ldc4=None):
    """layout: first letter A ('n': sAk == 1, rows of K; 't': sAm == 1, stored [K, M]), second letter B ('t':
    sBk == 1, stored [N, K]; 'n': sBn == 1, stored [K, N]) — "nt" and "tn" are the fast paths' layouts"""
    # ldc4: an fp32 C (with its aux) whose ldc is 4 (mod 8): legal for every fp32 route but the 256-wide NT kernels,
    # which refuse it (the product then runs on the 128-tile kernel); by default every other seed
    return dict(M=M, N=N, K=Kdim, layout=layout, ab=ab, c=c, epi=epi, alpha=float(alpha), acc=acc, colsum=colsum,
                colstats=colstats, c_null=c_null, relu=relu, aux=aux, bias=bias, batch=tuple(batch), family=family,
                cus=cus, seed=seed, ldc4=(c == F32 and seed % 2 == 1) if ldc4 is None else bool(ldc4))


def describe(s):
    t = lambda d: "bf16" if d == BF else "fp32"
    extra = "".join(" " + n for n in ("acc", "colsum", "colstats", "c_null", "relu", "ldc4") if s[n])
    return "%s %dx%dx%d %s %s->%s %s alpha %g%s%s cus %d" % (
        s["family"], s["M"], s["N"], s["K"], s["layout"], t(s["ab"]), t(s["c"]), EPI_NAMES[s["epi"]], s["alpha"], extra,
        " batch %dx%d" % s["batch"] if s["batch"] != (1, 1) else "", s["cus"])


_POOL = {}


def _pool(kind):
    """one fixed stream of 2^24 variates per kind; a tensor is a slice of it (cheap for the large shapes)"""
    if kind not in _POOL:
        g = torch.Generator("cpu").manual_seed({"n": 20240, "u": 20241}[kind])
        _POOL[kind] = torch.randn(1 << 24, generator=g) if kind == "n" else torch.rand(1 << 24, generator=g)
    return _POOL[kind]


class _Draw:
    def __init__(self, seed):
        self.pos = (seed * 7919 + 13) % (1 << 22)

    def _take(self, kind, shape):
        n = 1
        for v in shape:
            n *= v
        p = _pool(kind)
        if self.pos + n > p.numel():
            self.pos = (self.pos * 31 + 17) % max(p.numel() - n, 1)
        t = p[self.pos:self.pos + n].reshape(shape).clone()
        self.pos += n + 61
        return t

    def randn(self, *shape):
        return self._take("n", shape)

    def rand(self, *shape):
        return self._take("u", shape)

    def ints(self, lo, hi, *shape):      # integers in [lo, hi)
        return torch.floor(self._take("u", shape) * (hi - lo) + lo).clamp_(lo, hi - 1)


SPECIAL_U = (0.0, -0.0, 2.0 ** -12, -2.0 ** -12, 16.0, -16.0, 30.0, -30.0, 1e4, -1e4)


def sweep(rows, cols, dtype):
    """[rows, cols] values that sweep [-12, 12] densely (row-major) with the special arguments in row 0"""
    t = torch.linspace(-12.0, 12.0, max(rows * cols, 1))[:rows * cols].reshape(rows, cols).clone()
    n = min(len(SPECIAL_U), cols) if rows else 0
    if n:
        t[0, :n] = torch.tensor(SPECIAL_U[:n])
    return t.to(dtype).float()


def needs(s):
    """which optional operands the call of spec `s` reads"""
    epi = s["epi"]
    return {"residual": epi == BIAS_RESIDUAL, "aux": epi in (DGELU, MUL_AUX, ADD_AUX) or (epi == AFFINE and s["aux"]),
            "scale": epi == AFFINE, "c0": bool(s["acc"]), "cs0": bool(s["acc"] and s["colsum"])}


def make_case(s):
    """the operands of spec `s` as logical fp32 CPU tensors holding values of the declared types, and their guarded
    windows (`win`).  A [b1, b2, M, K], B [b1, b2, K, N]"""
    M, N, Kd, fam = s["M"], s["N"], s["K"], s["family"]
    b1, b2 = s["batch"]
    d = _Draw(s["seed"] + 131 * M + 17 * N + 7 * Kd + 1009 * FAMILIES.index(fam) + 3 * s["epi"])
    ab, ct = s["ab"], s["c"]
    q = lambda t, dt: t.to(dt).float()
    nd = needs(s)
    mr, ma, mc = (M if nd["residual"] else 0), (M if nd["aux"] else 0), (M if nd["c0"] else 0)     # rows of what is not read: none
    if fam == "integers":
        A = d.ints(-2, 4, b1, b2, M, Kd)
        B = d.ints(-3, 3, b1, b2, Kd, N) / 8
        bias = d.ints(-64, 65, N) / 16
        res = d.ints(-64, 65, mr, N) / 16
        aux = d.ints(-8, 9, ma, N) / 4
        scale = d.ints(-8, 9, N) / 4
        c0 = d.ints(-32, 33, b1, b2, mc, N) / 4
        cs0 = d.ints(-32, 33, M) / 4
    else:
        kk = max(Kd, 1)
        if fam == "onehot":
            A = torch.zeros(b1, b2, M, Kd)
            if Kd:
                A[..., torch.arange(M), torch.arange(M) % Kd] = 1.0
            B = sweep(Kd, N, ab).expand(b1, b2, Kd, N).clone()
        elif fam == "offset":
            A = 0.25 + 0.5 * d.randn(b1, b2, M, Kd).abs()
            B = (0.5 + d.randn(b1, b2, Kd, N).abs()) * kk ** -0.5
        else:
            A = 0.5 * d.randn(b1, b2, M, Kd)
            B = d.randn(b1, b2, Kd, N) * kk ** -0.5
            if fam == "massive" and Kd >= 2:
                A[..., 1 % Kd] *= 100.0
                A[..., Kd - 2] *= 100.0
            if fam == "cancel":
                h = Kd // 2
                A, B = q(A, ab), q(B, ab)
                A[..., h:2 * h] = A[..., :h]
                B[..., h:2 * h, :] = -B[..., :h, :]
                if Kd % 2:
                    A[..., Kd - 1] = 0.0
        bias = 0.1 * d.randn(N)
        if fam == "onehot" and N:         # fills the gaps of the grid; column 0 keeps the special arguments exact
            bias = (torch.arange(N) % 16).float() * (24.0 / max(Kd * N, 1) / 16.0)
            bias[:len(SPECIAL_U)] = 0.0
        res = d.randn(mr, N)
        aux = d.randn(ma, N)
        scale = d.randn(N)
        c0 = d.randn(b1, b2, mc, N)
        cs0 = d.randn(M)
    if N > 0:
        scale[0] = -scale[0].abs() - 0.25
    if N > 1:
        scale[1] = 0.0
    if s["epi"] == DGELU and fam != "integers":
        aux = sweep(ma, N, ct)
    case = {"spec": s, "A": q(A, ab), "B": q(B, ab), "bias": bias, "residual": res, "aux": q(aux, ct), "scale": scale,
            "c0": q(c0, ct) if s["acc"] else None, "cs0": cs0 if (s["acc"] and s["colsum"]) else None}
    if fam == "onehot" and s["epi"] in (MUL_AUX, ADD_AUX, AFFINE):
        case["aux"] = sweep(ma, N, ct)
    _windows(case)
    return case


def _windows(case):
    """lays the operands between NaN bands and the outputs' initial contents into sentinel-filled buffers"""
    s = case["spec"]
    M, N, Kd = s["M"], s["N"], s["K"]
    b1, b2 = s["batch"]
    nan = float("nan")
    la, lb = s["layout"]
    w = {}
    # A: rows of K (lda = K rounded up to 8, + 8) or stored [K, M]; batches with strides of their own
    ra, ca = (M, Kd) if la == "n" else (Kd, M)
    lda = _up8(ca) + 8
    blk = ra * lda + 24
    sa = (3 * blk + 40, blk, lda, 1) if la == "n" else (3 * blk + 40, blk, 1, lda)
    w["A"] = Window((b1, b2, M, Kd), sa, s["ab"], nan, lda).set(case["A"])
    rb, cb = (N, Kd) if lb == "t" else (Kd, N)
    ldb = _up8(cb) + 16
    blk = rb * ldb + 8
    sb = (3 * blk + 8, blk, 1, ldb) if lb == "t" else (3 * blk + 8, blk, ldb, 1)
    w["B"] = Window((b1, b2, Kd, N), sb, s["ab"], nan, ldb).set(case["B"])
    ldc = ldc_of(s)
    ldr = ldc + 4
    blk = M * ldc + 16
    sc = (3 * blk + 24, blk, ldc, 1)
    w["bias"] = Window((N,), (1,), F32, nan).set(case["bias"])
    w["scale"] = Window((N,), (1,), F32, nan).set(case["scale"])
    nd = needs(s)
    w["residual"] = Window((M if nd["residual"] else 0, N), (ldr, 1), F32, nan, ldr).set(case["residual"])
    w["aux"] = Window((M if nd["aux"] else 0, N), (ldc, 1), s["c"], nan, ldc).set(case["aux"])
    w["C"] = Window((b1, b2, M, N), sc, s["c"], SENTINEL, ldc)
    if case["c0"] is not None:
        w["C"].set(case["c0"])
    w["out2"] = Window((M if "out2" in outputs_of(s) else 0, N), (ldc, 1), s["c"], SENTINEL, ldc)
    w["colsum"] = Window((M if s["colsum"] else 0,), (1,), F32, SENTINEL)
    if case["cs0"] is not None:
        w["colsum"].set(case["cs0"])
    w["colstats"] = Window(((M + 127) // 128 if s["colstats"] else 0, 2, N), (2 * N, N, 1), F32, SENTINEL)
    case["win"] = w
    case["ldc"], case["ldr"] = ldc, ldr


def outputs_of(s):
    o = [] if s["c_null"] else ["C"]
    if s["epi"] in (BIAS_GELU, BIAS_GELU_GRAD):
        o.append("out2")
    if s["colsum"]:
        o.append("colsum")
    if s["colstats"]:
        o.append("colstats")
    return o


def to_device(case, device):
    c = dict(case)
    for n in ("A", "B", "bias", "residual", "aux", "scale", "c0", "cs0"):
        if c[n] is not None:
            c[n] = c[n].to(device)
    return c


# ------------------------------------------------------------------ GELU forms
RSQRT2, RSQRT2PI = 0.70710678118654752440, 0.39894228040143267794


def gelu64(u):
    u = u.to(F64)
    return 0.5 * u * torch.erfc(-u * RSQRT2)


def dgelu64(u):
    u = u.to(F64)
    return 0.5 * torch.erfc(-u * RSQRT2) + u * torch.exp(-0.5 * u * u) * RSQRT2PI


def gelu_erf32(x):
    """gemm.hip gelu_f / dgelu_f in fp32 torch -> (gelu, gelu')"""
    x = x.float()
    cdf = 0.5 * (1.0 + torch.erf(x * RSQRT2))
    return x * cdf, cdf + x * (RSQRT2PI * torch.exp(-0.5 * x * x))


def gelu_poly32(x):
    """common.h gelu_parts_fast (A&S 7.1.26) in fp32 torch -> (gelu, gelu')"""
    x = x.float()
    e = torch.exp(-0.5 * x * x)
    t = 1.0 / (1.0 + (0.3275911 * RSQRT2) * x.abs())
    poly = ((((1.061405429 * t - 1.453152027) * t + 1.421413741) * t - 0.284496736) * t + 0.254829592) * t
    cdf = 0.5 + 0.5 * torch.copysign(1.0 - poly * e, x)
    return x * cdf, cdf + x * e * RSQRT2PI


def gelu_tanh32(x):
    x = x.float()
    t = torch.tanh(0.7978845608028654 * (x + 0.044715 * x ** 3))
    return 0.5 * x * (1 + t), 0.5 * (1 + t) + 0.5 * x * (1 - t * t) * 0.7978845608028654 * (1 + 3 * 0.044715 * x * x)


def _gen_gelu_table():
    tools = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools")
    if tools not in sys.path:
        sys.path.insert(0, tools)
    import gen_gelu_table
    return gen_gelu_table


def gelu_table32(x):
    """gelu_table.h as tools/gen_gelu_table.emulate reads it: (gelu, gelu') as the bf16 values the kernel stores"""
    import numpy as np
    gt = _gen_gelu_table()
    xn = x.detach().float().cpu().contiguous().numpy()
    d, g = gt.emulate(xn.reshape(-1))
    f = lambda b: torch.from_numpy((b.astype(np.uint32) << 16).view(np.float32).copy()).reshape(x.shape).to(x.device)
    return f(g), f(d)


GELU_FORMS = {"erf": gelu_erf32, "poly": gelu_poly32, "table": gelu_table32}


def _table_test():
    import test_gpu_gelu_table
    return test_gpu_gelu_table


def table_bound_g(u):
    """`bound_g` of tests/test_gpu_gelu_table.py (the bound test_gelu_table_accuracy_cpu asserts) for fp64
    pre-activations u"""
    u = u.to(F64)
    b = _table_test().bound_g(u.detach().cpu().numpy(), gelu64(u).detach().cpu().numpy())
    return torch.from_numpy(b).to(u.device)


def gelu_grid():
    return torch.cat([torch.linspace(-20.0, 20.0, 400001), torch.tensor(SPECIAL_U)]).float()


def measure_gelu_constants(form, device="cpu"):
    """worst |form(u) - exact| / (|u| 2^-24) for gelu and / 2^-24 for gelu' over gelu_grid()"""
    u = gelu_grid().to(device)
    g, d = GELU_FORMS[form](u)
    eg = (g.double() - gelu64(u)).abs() / (u.double().abs() * EPS32)
    eg = torch.where(u == 0, torch.zeros_like(eg), eg)
    ed = (d.double() - dgelu64(u)).abs() / EPS32
    return float(eg.max()), float(ed.max())


def approx_terms(form, u, out_dtype):
    """(A_g, A_d, u_g, u_d): the approximation terms of gelu(u) / gelu'(u) and the output-rounding factors that go
    with them (the table's bounds contain the rounding)"""
    a = u.abs()
    if form == "table":
        return table_bound_g(u), torch.full_like(a, _table_test().DGELU_ABS), 0.0, 0.0
    cg, cd = GELU_C[form]
    return cg * a * EPS32, torch.full_like(a, cd * EPS32), u_of(out_dtype), u_of(out_dtype)


# ------------------------------------------------------------------ routing (labels; splits and GELU form)
def route(s, cus=None):
    """the dispatch of ssl4gie_gemm for spec `s` in the default environment, as read from gemm.hip (nt_ok, tn_ok,
    tn_splits, launch_slab_reduce), gemm_nt256.hip (nt256_ok, nt256_pick_nj, the launch) and gemm_tn256.hip
    (tn256_ok, ssl4gie_internal_tn256_splits with TN_SPLIT_LONE)"""
    cus = cus or s["cus"]
    M, N, Kd, epi = s["M"], s["N"], s["K"], s["epi"]
    r = {"kind": "generic", "splits": 1, "gelu": "erf"}
    one = s["batch"] == (1, 1)
    bf = s["ab"] == BF
    if M == 0 or N == 0:
        return r
    nt = (bf and one and s["layout"] == "nt" and Kd % 64 == 0 and Kd >= 64 and N % 4 == 0 and
          (s["c"] == F32 or epi == BIAS_RESIDUAL or (N % 8 == 0 and not s["acc"])))
    if nt:
        r["gelu"] = "poly"
        big = N % 8 == 0 and ldc_of(s) % 8 == 0
        if s["colstats"] and not (s["c"] == BF and epi == NONE and not s["acc"]):
            big = False
        elif epi == AFFINE:
            big = big and s["c"] == BF and not s["acc"]
        elif big and s["c"] == BF and (epi == BIAS_RESIDUAL or s["acc"]):
            big = False
        elif big and s["c"] == F32 and epi in (BIAS_GELU, DGELU, BIAS_GELU_GRAD, MUL_AUX, ADD_AUX):
            big = False
        elif big and not (epi == ADD_AUX or s["colstats"]):
            big = -(-M // 256) * -(-N // 256) >= 128
        if not big:
            tiles = -(-M // 128) * -(-N // 128)
            r.update(kind="nt128", tiles=tiles, wgs=min(tiles, 2 * cus))
            return r
        tm = -(-M // 256)
        r256, r192 = -(-tm * -(-N // 256) // cus), -(-tm * -(-N // 192) // cus)
        nj = 3 if r192 * 0.78 < r256 else 4
        if N <= 128 and s["c"] == BF and epi in (NONE, BIAS, ADD_AUX, AFFINE):
            nj = 2
        tiles = tm * -(-N // (64 * nj))
        wgs = min(tiles, cus)
        if tiles > cus:
            wgs = -(-tiles // -(-tiles // cus))
        table = nj == 4 and s["c"] == BF and epi in (BIAS_GELU, BIAS_GELU_GRAD)
        r.update(kind="nt256", nj=nj, tiles=tiles, wgs=wgs, ragged=bool(M % 256 or N % (64 * nj)),
                 streaming=M >= 16384 and not s["colstats"], table=table, stats=bool(s["colstats"]))
        if table:
            r["gelu"] = "table"
        return r
    tn = (bf and s["c"] == F32 and one and s["layout"] == "tn" and M % 8 == 0 and N % 8 == 0 and epi == NONE and
          Kd > 0 and M >= 8 and N >= 8)
    if tn:
        if Kd % 64 == 0 and Kd >= 1024 and M * N >= 65536:
            tiles, nkt = -(-M // 256) * -(-N // 256), Kd // 64
            sp = max(1, min((cus * 75 // 100 + tiles // 2) // tiles, nkt // 8, 256))
            r.update(kind="tn256", splits=sp, partial=bool(M % 256 or N % 256), fused_colsum=bool(s["colsum"]),
                     reduce="none" if sp == 1 else ("plain" if s["colsum"] or sp < 32 else "wide4" if sp < 128 else "wide16"))
            return r
        tiles, nkt = -(-M // 128) * -(-N // 128), -(-Kd // 64)
        sp = max(1, min(-(-1024 // tiles), nkt // 4, 256))
        r.update(kind="tn128", splits=sp,
                 reduce="none" if sp == 1 else ("plain" if sp < 32 else "wide4" if sp < 128 else "wide16"))
        return r
    return r


def many_splits(cases, cus, entry):
    """the split count of one launch of several TN products with the same K (entry "pair": ssl4gie_gemm_tn_pair,
    "group": ssl4gie_gemm_tn_group) in the default environment, as read from gemm_tn256.hip
    (ssl4gie_internal_tn256_splits: TN_SPLIT_PAIR aims at 75 % of the CUs, TN_SPLIT_GROUP at all of them and takes
    whole-K tiles once they cover 70 % of the CUs; both keep 8 K-tiles per split and stop at 64)"""
    specs = [c["spec"] for c in cases]
    tiles = sum(-(-s["M"] // 256) * -(-s["N"] // 256) for s in specs)
    if entry == "group" and tiles * 10 >= cus * 7:
        return 1
    fill = 75 if entry == "pair" else 100
    return max(1, min((cus * fill // 100 + tiles // 2) // tiles, specs[0]["K"] // 64 // 8, 64))


def route_label(r):
    if r["kind"] == "nt256":
        return "nt256 nj%d%s%s%s%s" % (r["nj"], " ragged" if r["ragged"] else " full", " streaming" if r["streaming"] else "",
                                      " table" if r["table"] else "", " stats" if r["stats"] else "")
    if r["kind"] == "tn256":
        return "tn256 %s splits %d reduce %s%s" % ("partial" if r["partial"] else "ksplit", r["splits"], r["reduce"],
                                                  " fused-colsum" if r["fused_colsum"] else "")
    if r["kind"] == "tn128":
        return "tn128 splits %d reduce %s" % (r["splits"], r["reduce"])
    return r["kind"]


# ------------------------------------------------------------------ fp64 reference and checks
def reference(case, got_c=None):
    """name -> (ref, mag) in fp64 for C / out2 / colsum (+ 'u': the fp64 pre-activation and its mag, 'acc')"""
    s = case["spec"]
    A, B = case["A"].to(F64), case["B"].to(F64)
    acc = A @ B
    mag_acc = A.abs() @ B.abs()
    al = s["alpha"]
    epi = s["epi"]
    v, mag = al * acc, abs(al) * mag_acc
    o = {"acc": acc, "mag_acc": mag_acc}
    bias = case["bias"].to(F64) if s["bias"] else torch.zeros_like(case["bias"], dtype=F64)
    if epi in (BIAS, BIAS_GELU, BIAS_RESIDUAL, BIAS_GELU_GRAD):
        v, mag = v + bias, mag + bias.abs()
    if epi == BIAS_RESIDUAL:
        r = case["residual"].to(F64)
        v, mag = v + r, mag + r.abs()
    aux = case["aux"].to(F64) if needs(s)["aux"] else None
    if epi == MUL_AUX:
        v, mag = v * aux, mag * aux.abs()
    if epi == DGELU:
        f = dgelu64(aux)
        o["pre"] = (v.abs(), mag)
        v, mag = v * f, mag * f.abs()
    if epi == ADD_AUX:
        v, mag = v + aux, mag + aux.abs()
    if epi == AFFINE:
        sc = case["scale"].to(F64)
        v, mag = v * sc + bias, mag * sc.abs() + bias.abs()
        if s["aux"]:
            v, mag = v + aux, mag + aux.abs()
        if s["relu"]:
            v = v.clamp_min(0)
    if s["acc"]:
        c0 = case["c0"].to(F64)
        v, mag = v + c0, mag + c0.abs()
    if epi in (BIAS_GELU, BIAS_GELU_GRAD):
        o["u"] = (v, mag)
        o["out2"] = gelu64(v)
        o["C"] = (v, mag) if epi == BIAS_GELU else (dgelu64(v), mag)
    else:
        o["C"] = (v, mag)
    if s["colsum"]:
        cs, mcs = A.sum(-1).reshape(-1), A.abs().sum(-1).reshape(-1)
        if case["cs0"] is not None:
            cs, mcs = cs + case["cs0"].to(F64), mcs + case["cs0"].to(F64).abs()
        o["colsum"] = (cs, mcs)
    return o


def ref_colstats(c_bf16, M, N):
    """fp64 sums / sums of squares per 128-row block of the returned bf16 C [M, N] -> ([R, 2, N], mags [R, 2, N])"""
    y = c_bf16.to(F64).reshape(M, N)
    R = (M + 127) // 128
    pad = torch.zeros(R * 128 - M, N, dtype=F64, device=y.device)
    y = torch.cat([y, pad]).reshape(R, 128, N)
    s1, s2, a1 = y.sum(1), (y * y).sum(1), y.abs().sum(1)
    return torch.stack([s1, s2], 1), torch.stack([a1, s2], 1)


def round_to(ref64, dtype):
    return ref64.float().to(dtype)


def check_case(case, outs, splits=1, form="erf", k=None, measure=False, tag=None, generic=False):
    """every check on the output buffers `outs` (name -> flat buffer laid out as case['win'][name]) of one case.
    splits / form: of the route that produced them (the class of k, the GELU approximation term)"""
    s = case["spec"]
    rep = Report(k, tag or describe(s), measure)
    win = case["win"]
    M, N = s["M"], s["N"]
    kn = acc_class(s["K"], splits, bool(generic))
    kk = rep.k[kn]
    exact = s["family"] == "integers"
    ct = s["c"]
    got = {}
    for name in ("C", "out2", "colsum", "colstats"):
        if name in outs:
            buf = outs[name]
            if name in outputs_of(s):
                got[name] = win[name].view(buf)
            rep.guard(name, buf, win[name])         # an output that is not wanted must stay untouched altogether
            if name not in outputs_of(s) and bool((win[name].view(buf) != win[name].view().to(buf.device)).any()):
                rep.failed_names.add("guard")
                rep.failed.append("%s guard: %s was written though the call does not produce it" % (rep.tag, name))
    if M == 0 or N == 0:
        return rep
    dev = next(iter(got.values())).device if got else case["A"].device
    ref = reference(case if case["A"].device == dev else to_device(case, dev))
    epi = s["epi"]
    if "C" in got:
        r, mag = ref["C"]
        if epi in (BIAS_GELU, BIAS_GELU_GRAD):
            u64, mag_u = ref["u"]
            ag, ad, ug, ud = approx_terms(form, u64, ct)
            b_u = kk * EPS32 * mag_u
            if epi == BIAS_GELU:
                rep.ratio("C", got["C"], u64, mag_u, u_of(ct), kname=kn)
            else:
                rep.ratio("C", got["C"], r, mag_u, ud, slack=ad, kname=kn, kscale=0.80)
            rep.ratio("out2", got["out2"], ref["out2"], mag_u, ug, slack=ag, kname=kn, kscale=1.13)
        elif epi == DGELU:
            pre, mag_pre = ref["pre"]
            cd = GELU_C["poly" if form == "table" else form][1]
            rep.ratio("C", got["C"], r, mag, u_of(ct), slack=(pre + kk * EPS32 * mag_pre) * cd * EPS32, kname=kn)
        else:
            rep.ratio("C", got["C"], r, mag, u_of(ct), kname=kn)
            if exact:
                rep.same("C", got["C"], round_to(r, ct), "not the fp64 value rounded once to the output type")
    if "colsum" in got:
        r, mag = ref["colsum"]
        rep.ratio("colsum", got["colsum"], r, mag)
        if exact:
            rep.same("colsum", got["colsum"].to(F64), r, "not the exact sum")
    if "colstats" in got and "C" in got:
        r, mag = ref_colstats(got["C"], M, N)
        rep.ratio("colstats", got["colstats"], r, mag)
        if exact:       # sums of at most 128 bf16 values in sixteenths below 2^9: exact in fp32 in any order
            rep.same("colstats", got["colstats"][:, 0].to(F64), r[:, 0], "column sums not exact")
    return rep


def old_rel_err(case, outs, name="C"):
    """the global norm the existing tests judge by: |got - ref| / |ref| over the whole matrix"""
    ref = reference(case)
    r = ref[name][0] if isinstance(ref[name], tuple) else ref[name]
    g = case["win"][name].view(outs[name]).to(F64)
    return float((g - r).norm() / r.norm().clamp_min(1e-300))


# ------------------------------------------------------------------ the fp32 emulation and its wrong variants
# name -> the check that must fail
MUTATIONS = {
    "bias_before_alpha": "C",
    "alpha_dropped": "C",
    "bias_twice": "C",
    "bias_shifted_4_columns_last_tile": "C",
    "residual_read_with_ldc": "C",
    "aux_read_with_stride_n": "C",
    "accumulate_ignored": "C",
    "alpha_on_old_c": "C",
    "last_k_chunk_dropped": "C",
    "ragged_k_tail_not_zeroed": "C",
    "chunk_from_neighbour": "C",
    "last_row_duplicated": "C",
    "slab_dropped": "C",
    "slab_twice": "C",
    "colsum_ignores_accumulate": "colsum",
    "colstats_from_unrounded": "colstats",
    "colstats_with_clamped_rows": "colstats",
    "colstats_blocks_of_256": "colstats",
    "relu_before_aux": "C",
    "shift_before_scale": "C",
    "tanh_gelu": "out2",
    "dgelu_times_gelu": "C",
    "bf16_truncated": "C",
    "store_past_n": "guard",
}


def _truncate_bf16(t):
    return (t.float().contiguous().view(torch.int32) & -65536).view(torch.float32).to(BF)


def emu_acc(A, B, splits=1, generic=False, mut=None):
    """the accumulators in fp32: A [.., M, K], B [.., K, N] fp32 tensors of operand values"""
    Kd = A.shape[-1]
    shape = A.shape[:-1] + B.shape[-1:]
    zero = lambda: torch.zeros(shape, dtype=F32, device=A.device)
    A64, B64 = A.to(F64), B.to(F64)
    if generic:                 # f32 MFMA: a k-ordered fmaf chain
        acc = zero()
        for kq in range(Kd - 1 if mut == "last_k_chunk_dropped" else Kd):
            acc = (acc.double() + A64[..., kq:kq + 1] * B64[..., kq:kq + 1, :]).float()
        return acc
    nkt = -(-Kd // 64)
    parts = []
    for sp in range(splits):
        acc = zero()
        c0, c1 = 2 * (nkt * sp // splits), 2 * (nkt * (sp + 1) // splits)
        if mut == "last_k_chunk_dropped" and sp == splits - 1:
            c1 = min(c1, -(-Kd // 32)) - 1
        for ch in range(c0, c1):
            lo, hi = 32 * ch, min(32 * ch + 32, Kd)
            if lo >= hi:
                break
            p = A64[..., lo:hi] @ B64[..., lo:hi, :]
            if mut == "ragged_k_tail_not_zeroed" and hi == Kd and Kd % 64:     # rows past K hold the clamped row K - 1
                p = p + (64 - Kd % 64) * A64[..., Kd - 1:Kd] * B64[..., Kd - 1:Kd, :]
            acc = (acc.double() + p).float()
        parts.append(acc)
    if mut == "slab_dropped" and splits > 1:
        parts.pop(splits // 2)
    if mut == "slab_twice" and splits > 1:
        parts.insert(splits // 2, parts[splits // 2])
    acc = parts[0]
    for p in parts[1:]:
        acc = acc + p
    return acc


def emulate(case, splits=1, generic=False, form="erf", mut=None, blocks=128):
    """the outputs of `case` by the fp32 emulation, as flat buffers laid out like case['win'] (name -> buffer);
    `mut`: one of MUTATIONS, a deliberately wrong variant"""
    s = case["spec"]
    M, N, Kd, epi, al = s["M"], s["N"], s["K"], s["epi"], s["alpha"]
    win = case["win"]
    dev = case["A"].device
    ct = s["c"]
    acc = emu_acc(case["A"], case["B"], splits, generic, mut)
    alpha = 1.0 if mut == "alpha_dropped" else al
    bias = case["bias"].float() if s["bias"] else torch.zeros(N, device=dev)
    nd = needs(s)
    aux = case["aux"].float() if nd["aux"] else None
    if mut == "aux_read_with_stride_n" and nd["aux"]:
        w = win["aux"]
        aux = torch.as_strided(w.buf, (M, N), (N, 1), w.off).float().to(dev)
    res = case["residual"].float()
    if mut == "residual_read_with_ldc" and nd["residual"]:
        w = win["residual"]
        res = torch.as_strided(w.buf, (M, N), (case["ldc"], 1), w.off).float().to(dev)
    bias_mn = bias.expand(M, N)
    if mut == "bias_shifted_4_columns_last_tile" and N > 4:      # the last 128 x 128 tile only
        m0, n0 = 128 * ((M - 1) // 128), 128 * ((N - 1) // 128)
        bias_mn = bias_mn.clone()
        bias_mn[m0:, n0:N - 4] = bias[n0 + 4:N]
    has_bias = epi in (BIAS, BIAS_GELU, BIAS_RESIDUAL, BIAS_GELU_GRAD)
    if mut == "bias_before_alpha" and has_bias:
        v = (acc + bias_mn) * alpha
    else:
        v = acc * alpha
        if has_bias:
            v = v + bias_mn * (2.0 if mut == "bias_twice" else 1.0)
    out2 = None
    if epi == BIAS_RESIDUAL:
        v = v + res
    elif epi == MUL_AUX:
        v = v * aux
    elif epi == DGELU:
        g, dg = GELU_FORMS["poly" if form == "table" else form](aux)
        v = v * (g if mut == "dgelu_times_gelu" else dg)
    elif epi == ADD_AUX:
        v = v + aux
    elif epi == AFFINE:
        sc = case["scale"].float()
        a = aux if s["aux"] else 0.0
        if mut == "shift_before_scale":
            v = (v + case["bias"].float()) * sc + a
        elif mut == "relu_before_aux" and s["relu"]:
            v = (v * sc + case["bias"].float()).clamp_min(0) + a
        else:
            v = v * sc + case["bias"].float() + a
        if s["relu"] and mut != "relu_before_aux":
            v = v.clamp_min(0)
    elif epi in (BIAS_GELU, BIAS_GELU_GRAD):
        g, dg = (gelu_tanh32 if mut == "tanh_gelu" else GELU_FORMS[form])(v)
        out2 = g
        if epi == BIAS_GELU_GRAD:
            v = dg
    if s["acc"] and mut != "accumulate_ignored":
        v = v + case["c0"].float() * (alpha if mut == "alpha_on_old_c" else 1.0)
    rnd = (lambda t: _truncate_bf16(t)) if (mut == "bf16_truncated" and ct == BF) else (lambda t: t.to(ct))
    c = rnd(v)
    if mut == "chunk_from_neighbour" and N >= 16:       # one 16-byte chunk (a row of 8 columns) of the last tile
        m0 = 128 * ((M - 1) // 128)
        c[..., m0, N - 8:N] = c[..., m0, N - 16:N - 8]
    if mut == "last_row_duplicated" and M > 1:
        c[..., M - 1, :] = c[..., M - 2, :]
    outs = {}
    for name in ("C", "out2", "colsum", "colstats"):
        outs[name] = win[name].buf.clone().to(dev)
    if not s["c_null"]:
        win["C"].view(outs["C"]).copy_(c)
        if mut == "store_past_n":
            w = win["C"]
            outs["C"][w.off + N:w.off + N + 8] = 1.0
    if out2 is not None:
        win["out2"].view(outs["out2"]).copy_(out2.reshape(M, N).to(ct))
    if s["colsum"]:
        cs = case["A"].float().sum(-1).reshape(-1)
        if case["cs0"] is not None and mut != "colsum_ignores_accumulate":
            cs = cs + case["cs0"].float()
        win["colsum"].view(outs["colsum"]).copy_(cs)
    if s["colstats"]:
        y = (v if mut == "colstats_from_unrounded" else c.float()).reshape(M, N)
        if mut == "colstats_blocks_of_256":
            blocks = 256
        R = (M + 127) // 128
        st = torch.zeros(R, 2, N, device=dev)
        for r in range(-(-M // blocks)):
            yb = y[blocks * r:blocks * (r + 1)]
            if mut == "colstats_with_clamped_rows" and yb.shape[0] < blocks:
                yb = torch.cat([yb, y[M - 1:M].expand(blocks - yb.shape[0], N)])
            st[r * blocks // 128, 0], st[r * blocks // 128, 1] = yb.sum(0), (yb * yb).sum(0)
        win["colstats"].view(outs["colstats"]).copy_(st)
    return outs


def emulate_and_check(case, cus=None, mut=None, measure=False, k=None):
    r = route(case["spec"], cus)
    outs = emulate(case, r["splits"], r["kind"] == "generic", r["gelu"], mut)
    return check_case(case, outs, r["splits"], r["gelu"], k=k, measure=measure, generic=r["kind"] == "generic"), outs


# ------------------------------------------------------------------ the case list of the GPU module
ALPHAS = (1.0, 0.5, -2.0, 0.75)
EXACT_EPIS = (NONE, BIAS, BIAS_RESIDUAL, MUL_AUX, ADD_AUX, AFFINE)
BIG_MACS = 1e8          # above this the fp64 reference is taken on the device


def families_for(epi, i=0):
    """gauss plus the exact families: integers where the epilogue has no transcendental, onehot where it has one
    (and for the affine map)"""
    f = ["gauss"]
    if epi in EXACT_EPIS:
        f.append("integers")
    if epi in (BIAS_GELU, DGELU, BIAS_GELU_GRAD, AFFINE):
        f.append("onehot")
    return f


def _alpha(i, family):
    if family == "onehot":      # u = B + bias: the special arguments are met exactly
        return 1.0
    return ALPHAS[i % 3] if family == "integers" else ALPHAS[i % 4]


GEN_MN = (1, 5, 63, 64, 65, 130)
GEN_K = (0, 1, 3, 15, 16, 17, 33, 100)
TYPE_PAIRS = ((F32, F32), (BF, BF), (BF, F32), (F32, BF))


def gpu_generic_specs():
    i = 0
    for ab, ct in TYPE_PAIRS:
        for layout in ("nt", "tn", "nn", "tt"):
            grp = "generic-%s%s-%s" % ("b" if ab == BF else "f", "b" if ct == BF else "f", layout)
            for ik, Kd in enumerate(GEN_K):
                for im, M in enumerate(GEN_MN):
                    N = GEN_MN[(im + ik + len(grp)) % 6]
                    epi = i % 7
                    for fam in families_for(epi):
                        acc = epi == NONE and i % 2 == 0
                        yield grp, spec(M, N, Kd, layout, ab, ct, epi, _alpha(i, fam), acc=acc,
                                        colsum=(layout[0] == "t" and i % 3 == 0), bias=(epi == BIAS or i % 5 != 0),
                                        family=fam, seed=i)
                    i += 1
            # two-level batches with strides of their own; the plain epilogue only
            for j, (M, N, Kd) in enumerate(((5, 65, 17), (64, 63, 33), (130, 5, 100))):
                for fam in ("gauss", "integers"):
                    yield grp, spec(M, N, Kd, layout, ab, ct, NONE, _alpha(j + 1, fam), acc=j == 1, batch=(2, 3),
                                    family=fam, seed=900 + j)
    # accumulation-length families on the generic kernel (a chain of K + 1 = 101 links: acc_L128)
    for fam in ("offset", "cancel", "massive"):
        for ab, ct in TYPE_PAIRS:
            yield "generic-families", spec(65, 63, 100, "nn", ab, ct, BIAS, 0.75, family=fam)


NT128_M = (1, 127, 128, 129, 250)
NT128_N = (8, 120, 136, 264)
NT128_K = (64, 128, 448)


def gpu_nt128_specs():
    i = 0
    for ct in (BF, F32):
        grp = "nt128-%s" % ("bf16" if ct == BF else "fp32")
        for epi in range(7):
            for im, M in enumerate(NT128_M):
                for jn, N in enumerate(NT128_N + ((12,) if ct == F32 or epi == BIAS_RESIDUAL else ())):
                    Kd = NT128_K[i % 3]
                    for fam in families_for(epi):
                        yield grp, spec(M, N, Kd, "nt", BF, ct, epi, _alpha(i, fam), acc=(ct == F32 and epi == NONE and i % 2 == 0),
                                        bias=(epi == BIAS or i % 4 != 0), family=fam, seed=i)
                    i += 1
        for fam in ("offset", "cancel", "massive"):
            yield grp, spec(129, 136, 448, "nt", BF, ct, BIAS, 0.75, family=fam)
            yield grp, spec(129, 136, 4096, "nt", BF, ct, NONE, 0.75, family=fam)
            yield grp, spec(33, 72, 32768, "nt", BF, ct, BIAS, 0.75, family=fam)
    # 25 tiles on 16 workgroups, one K-tile per tile: the next tile's operands and aux are in flight in the epilogue
    for ct in (BF, F32):
        for epi in range(7):
            for fam in families_for(epi):
                yield "nt128-rounds", spec(640, 640, 64, "nt", BF, ct, epi, _alpha(epi, fam), family=fam, cus=8, seed=epi)


NT256_M = (1, 127, 128, 129, 255, 256, 257, 300)
NT256_N = (8, 64, 72, 128, 136, 192, 200, 256, 264)
NT256_K = (64, 128, 320)


def _forced_variants(i):
    """the products only the 256-wide kernels have: (epi, colstats, c_null, relu, aux)"""
    return ((NONE, True, False, False, True), (ADD_AUX, False, False, False, True),
            (AFFINE, False, False, i % 2 == 0, i % 4 < 2))


def gpu_nt256_forced_specs():
    i = 0
    for im, M in enumerate(NT256_M):
        for jn, N in enumerate(NT256_N):
            Kd = NT256_K[(im + jn) % 3]
            for epi, stats, c_null, relu, aux in _forced_variants(i):
                for fam in families_for(epi):
                    yield "nt256-forced-M%d" % M, spec(M, N, Kd, "nt", BF, BF, epi, _alpha(i, fam), colstats=stats,
                                                       relu=relu, aux=aux, family=fam, seed=i)
            i += 1
    for fam in ("offset", "cancel", "massive"):
        yield "nt256-forced-families", spec(300, 264, 320, "nt", BF, BF, ADD_AUX, 0.75, family=fam)
        yield "nt256-forced-families", spec(300, 200, 4096, "nt", BF, BF, AFFINE, 0.75, relu=False, family=fam)
    # 256-wide tiles, two per workgroup
    for i in range(4):
        for epi, stats, c_null, relu, aux in _forced_variants(i):
            for fam in families_for(epi)[:2]:
                yield "nt256-forced-rounds", spec(1500, 512, 64 if i % 2 else 192, "nt", BF, BF, epi, _alpha(i, fam),
                                                  colstats=stats, relu=relu, aux=aux, family=fam, cus=8, seed=i)


NT256_BIG = ((16383, 512), (16383, 768), (32513, 192), (32513, 200), (32513, 128),
             (16384, 512), (16384, 768), (32768, 192), (32768, 256), (32768, 128))


def gpu_nt256_big_specs():
    i = 0
    for M, N in NT256_BIG:
        for ct, epis in ((BF, (0, 1, 2, 4, 5, 6)), (F32, (0, 1, 3))):
            for epi in epis:
                Kd = (64, 192)[i % 2]
                for fam in families_for(epi)[:2]:
                    yield "nt256-%dx%d" % (M, N), spec(M, N, Kd, "nt", BF, ct, epi, _alpha(i, fam),
                                                       acc=(ct == F32 and epi == NONE and i % 2 == 0), family=fam, seed=i,
                                                       ldc4=False)      # the 256-wide kernels want ldc % 8 == 0
                i += 1
        if M >= 16384:      # the streaming-store twins of the epilogues only the 256-wide kernels have
            for epi, stats, c_null, relu, aux in _forced_variants(i)[1:]:
                for fam in families_for(epi)[:2]:
                    yield "nt256-%dx%d" % (M, N), spec(M, N, (64, 192)[i % 2], "nt", BF, BF, epi, _alpha(i, fam), relu=relu,
                                                       aux=aux, family=fam, seed=i)
                i += 1
    for fam in ("offset", "cancel", "massive"):
        yield "nt256-families", spec(16383, 512, 192, "nt", BF, BF, BIAS, 0.75, family=fam)


TN128_MN = (8, 72, 128, 136, 264)
TN128_K = (8, 64, 70, 257, 1000)


def _alpha_ne1(i, family):
    return (0.5, -2.0)[i % 2] if family == "integers" else (0.5, -2.0, 0.75)[i % 3]


def gpu_tn128_specs():
    """all with alpha != 1 and accumulate"""
    i = 0
    for im, M in enumerate(TN128_MN):
        for jn, N in enumerate(TN128_MN):
            Kd = TN128_K[(im + jn) % 5]
            for fam in ("gauss", "integers"):
                yield "tn128", spec(M, N, Kd, "tn", BF, F32, NONE, _alpha_ne1(i, fam), acc=True, colsum=i % 3 == 0,
                                    family=fam, seed=i)
            i += 1
    for j, Kd in enumerate((8192, 32768, 65536)):       # 32, 128, 256 slabs
        for fam in ("gauss", "integers", "offset", "cancel", "massive"):
            yield "tn128-slabs%d" % (Kd // 256), spec(64, 64, Kd, "tn", BF, F32, NONE, _alpha_ne1(j, fam), acc=True,
                                                      colsum=(j == 1 and fam == "gauss"), family=fam, seed=j)
    for fam in ("offset", "cancel", "massive"):
        yield "tn128", spec(72, 136, 448, "tn", BF, F32, NONE, 0.75, acc=True, family=fam)


# M N >= 65536 and K >= 1024, or the product stays on the 128-tile kernel.  The last two have six and nine tiles: at 8
# CUs they run whole-K (splits == 1: alpha and accumulate in the kernel's own epilogue), k-split and partial
TN256_SHAPES = ((256, 256, 1024), (272, 248, 1088), (512, 128, 2048), (256, 256, 16384), (512, 768, 1024), (520, 600, 1024))
TN256_CUS = (8, 64, 240, 256)


def gpu_tn256_specs():
    i = 0
    for M, N, Kd in TN256_SHAPES:
        for cus in TN256_CUS:
            for colsum, acc in ((False, False), (False, True), (True, False), (True, True)):
                fams = ("gauss", "integers") + (("offset", "cancel", "massive") if cus == 240 and colsum == acc else ())
                for fam in fams:
                    yield "tn256-%dx%dx%d" % (M, N, Kd), spec(M, N, Kd, "tn", BF, F32, NONE, _alpha(i + 1, fam), acc=acc,
                                                              colsum=colsum, family=fam, cus=cus, seed=i)
                i += 1


def gpu_specs(big=True):
    for g in (gpu_generic_specs, gpu_nt128_specs, gpu_nt256_forced_specs, gpu_tn128_specs, gpu_tn256_specs):
        yield from g()
    if big:
        yield from gpu_nt256_big_specs()


def groups(specs):
    return list(dict.fromkeys(g for g, _ in specs))


def macs(s):
    return float(s["M"]) * s["N"] * s["K"] * s["batch"][0] * s["batch"][1]


def measure_k_ref(device, big=True, log=print):
    """worst error / (2^-24 mag) per check and class of the emulation over the GPU module's case list (the pair /
    group products are the TN shapes again)"""
    worst = {}
    for grp, s in gpu_specs(big):
        if macs(s) > BIG_MACS and str(device) == "cpu":
            continue
        case = to_device(make_case(s), device)
        rep, _ = emulate_and_check(case, measure=True)
        for n, v in rep.worst.items():
            if v > worst.get(n, 0.0):
                worst[n] = v
                log("k_ref %s = %.3f at %s: %s" % (n, v, grp, describe(s)))
    return worst
