"""fp64 references of the loss kernels of loss_ops.hip (ssi_loss, dice_loss, infonce_loss, cross_entropy,
soft_cross_entropy in both forms, bt_loss) and the per-element checks that pin those kernels to them
(tests/test_gpu_loss_kernels.py; proof that the checks bite: tests/test_loss_checks_cpu.py).  bt_loss_grad is held bit
for bit by tests/test_gpu_loss_heads.py, which also runs D = 1025 and 1028.

References: plain torch on the CPU in float64, from exactly the fp32 bits the kernel is handed (alpha, T, lambda,
smooth and F.normalize's eps as rounded to fp32).  Values are scalars, gradients come from autograd on the fp64
formulation, the upstream gradient is 1 (the wrappers' scaling is checked in the GPU module).
    ssi_loss             compute_scale_and_shift, mse_loss and gradient_loss of ssl4gie_amd/losses.py, written out again
                         (`ssi_formula`): scales k in 0..scales-1 on [:, ::2^k, ::2^k], batch-based reduction
    dice_loss            SoftDiceLoss.forward's torch branch
    infonce_loss         normalize, product, cross_entropy x 2T, labels arange + off
    cross_entropy        F.cross_entropy(weight=...)
    soft_cross_entropy   finetune_checks.soft_target_ce / label_smoothing_ce
    bt_loss              (diag - 1)^2.sum() + lambda (c^2.sum() - diag^2.sum())

Bounded checks, per output element: |got - ref| <= k 2^-24 mag (+ slack, see the sign terms), mag = the fp64 sum of the
ABSOLUTE values of the terms the kernel adds; where a term inherits the error of an earlier quantity, mag carries that
quantity's own delta (written d(x) below: the size, in units of 2^-24, of the error x may have).
  ssi.  Per image, over the valid pixels m = t > 0: a00 = sum p^2, a01 = sum p, n = sum 1, b0 = sum p t, b1 = sum t,
  and the abs-sums S1 = sum |p|, Sb0 = sum |p t| (a00, n and b1 are their own).  det = a00 n - a01^2,
  s = (n b0 - a01 b1) / det, h = (a00 b1 - a01 b0) / det.  A product x y errs by d(x) |y| + |x| d(y) + |x y|:
      d(det) = 2 a00 n + 2 S1^2               the cancellation of the determinant sits here
      d(s)   = (2 n Sb0 + 3 S1 b1 + |s| d(det)) / |det| + |s|
      d(h)   = (3 S1 Sb0 + 3 a00 b1 + |h| d(det)) / |det| + |h|
      d(d_i) = m (|p| d(s) + d(h) + |s p| + |h| + |t|),  d_i = m (s p + h - t)
    ssi_loss   sum m (d^2 + 2 |d| d(d)) / 2M + alpha sum_k sum_pairs (|e| + d(d_i) + d(d_j)) / M_k, e = d_j - d_i
    ssi_dpred  the closed form of pass C, g s + G1 ds/dp + G0 dh/dp (equal to autograd to 1e-12 of the largest
               gradient, asserted in the CPU module), with
                   g_i = d_i / M + alpha sum_k (sum of +-sign(e) over the pairs of i) / M_k
                   mag(g_i) = (|d_i| + d(d_i)) / M + alpha sum_k (pairs of i) / M_k
                   G0 = sum g, G1 = sum g p,  mag(G0) = sum mag(g), mag(G1) = sum mag(g) |p|
                   dd = 2 n p - 2 a01, mag(dd) = 2 n |p| + 2 S1
                   ds/dp = (n t - b1 - s dd) / det
                   mag(ds/dp) = (n t + b1 + |s| mag(dd) + d(s) |dd| + |ds/dp| d(det)) / |det| + |ds/dp|
                   dh/dp = (2 p b1 - b0 - a01 t - h dd) / det
                   mag(dh/dp) = (2 |p| b1 + Sb0 + S1 t + |h| mag(dd) + d(h) |dd| + |dh/dp| d(det)) / |det| + |dh/dp|
               mag = mag(g) |s| + |g| d(s) + mag(G1) |ds/dp| + |G1| mag(ds/dp) + mag(G0) |dh/dp| + |G0| mag(dh/dp).
               On well-conditioned inputs this bound is honest but loose (the fp32 torch formulation sits at k_ref
               below 1); on nearly constant predictions (`narrow`) it is dominated by d(det) / |det|, the
               conditioning of the 2 x 2 system, and says little more than that the kernel is no worse conditioned
               than the formula.  The tight pins are the exact families below.
  dice.  m1 = sigmoid(l) through the fast exponential, charged as head_y of map_checks: an error of the exponent's
  argument at the size of |l| moves m1 by m1 (1 - m1): d(m1) = m1 (1 - m1) |l| + m1.
      d(num) = sum (m1 + d(m1)) |t| + smooth,  d(den) = sum (m1^2 + 2 m1 d(m1)) + sum t^2 + smooth
      dice_loss     1 + mean_b [2 (d(num) / den + num d(den) / den^2) + |score|]
      dice_dlogits  (mag(ds) w + |ds| d(w)) / B,  ds = 2 t / den - 4 num m1 / den^2,  w = m1 (1 - m1),
                    mag(ds) = |2 t / den| + |4 num m1 / den^2| + 2 |t| d(den) / den^2
                              + 4 (d(num) m1 + num d(m1)) / den^2 + 8 num m1 d(den) / den^3,
                    d(w) = d(m1) + w  (1 - m1 is exact given m1, so it carries d(m1) whole: at l = 10 that is 2^-24
                    against w = 4.5e-5, and the kernel does have that error)
  nce.  q^ = q / max(|q|, eps).  A normalised element carries 2 roundings (the sum of squares at half weight through
  the root, the root, the division); a logit adds the product sum and the division by T:
      d(l_ij) = (6 / T) sum_c |q^_c k^_c|,   d(lse_i) = sum_j p_ij d(l_ij) + |max_j l_ij| + 1
      nce_loss   (2T / N) sum_i (d(lse_i) + d(l_i,label) + |lse_i| + |l_i,label|)
      d(p_ij) = p_ij (d(l_ij) + d(lse_i) + |l_ij - lse_i| + 1)
      g_ic = (2 / N) sum_j (p_ij - [j = label]) k^_jc,  mag(g_ic) = (2 / N) sum_j (3 |p_ij - [..]| + d(p_ij)) |k^_jc|
      nce_dq     dq = (g - q^ (q^ . g)) / |q|, a projection that cancels:
                 (mag(g_c) + |q^_c| sum_c' |q^_c'| (mag(g_c') + 2 |g_c'|) + 2 |q^_c (q^ . g)|) / |q| + 2 |dq_c|;
                 a query of norm <= eps: dq = g / eps, mag(g_c) / eps + |dq_c|
  ce, softce.  The log-sum-exp is charged at d(lse) = |max| + 1.
      ce_loss         sum_b w_b (|lse| + |x_t| + d(lse)) / sum w
      ce_dlogits      w_b (softmax + [c = t] + softmax (|x_c - lse| + d(lse))) / sum w
      softce_loss     mean_b [sum_c T_c (|logs| + |x_c - M|) + d(lse) sum_c T_c],  T_c = |t_c| for given targets and
                      4 |t_c| for the smoothed form (conf, off and their sum are rounded to fp32 on the way in)
      softce_dlogits  (softmax sum_c T_c + T_c + softmax sum_c |t_c| (|x_c - M - logs| + d(lse))) / B
  bt_loss   sum (c_ii - 1)^2 + lambda sum_{i != j} c_ij^2
  Underflow.  A result below the smallest normal 2^-126 may arrive as 0 (exp of an argument below -87, a product of two
  tiny factors): the softmax and sigmoid terms and every gradient's mag carry TINY = 2^-126 / 2^-24 = 2^-102.

Exact and near-exact checks.
  ssi_dyadic / ssi_dyadic_loss   the `dyadic` family: B = 3, 16 x 16, target a multiple of 1/4 in [1/4, 4], the left half
      of image 1 and the top half of image 2 masked (every M_k is a power of two: 512, 128, 32, 8), prediction +-1 in
      equal numbers over each image's valid pixels (a01 = 0, det = n^2), alpha = 0.5.  Every intermediate is exactly
      representable: fp32 torch gives the fp64 loss and all 768 gradient elements bit for bit (asserted in the CPU
      module), and neighbour pairs with a difference of exactly 0 exist, so sign(0) = 0 is tested.  Bounded with
      mag = |g s| + |G1 ds/dp| + |G0 dh/dp| only (nothing upstream may err) and no exemption.  The MI355X kernels gave
      every one of the 4 x 768 elements equal in value (a masked pixel may carry a zero of either sign), so the check
      is also a `same` check on the values; the Report counts the equal elements (`bit_equal`).
  ssi_zero   dpred is +-0 wherever the image's fp64 determinant is 0 or it has no valid pixel (`degenerate`: an
      image without a valid pixel, one with a single valid pixel, one with two valid pixels of equal prediction; also
      H = W = 1).  The kernel must give scale = shift = 0 there, whatever the compiler fused in the determinant.
  ssi_admit  the `perfect_fit` family (t = 2 p + 1, p a multiple of 1/64): every pair difference is rounding dust, its
      sign is nobody's to pin.  dpred must be finite and |dpred| <= the largest magnitude the formula admits (every
      sign term taken as 1: g_i <= |d_i| / M + alpha sum_k pairs_i / M_k) + k 2^-24 mag.  Its loss is held by ssi_loss.
  ce_zero    dlogits of a row whose class weight is 0 is +-0; dlogits at a -inf logit that is not the target is +-0
      with a finite loss (plain cross-entropy only: with soft targets torch gives NaN too).
  bt_exact   `integers`: c a multiple of 1/8 in [-2, 2].  Where both sums stay below 2^24 in units of 1/64 (asserted
      by the reference; D <= 256 here) the value is the fp64 value rounded once, up to the one product with lambda.

Sign terms of the SSI gradient.  sign(e) of a neighbour difference is discontinuous: a pixel is exempt from ssi_dpred
when one of its pairs has |e64| <= 16 2^-24 (d(d_i) + d(d_j)).  The exempt pixels are counted per case and the check
`ssi_exempt` fails when they exceed 2 % of the case's elements (a condition, not a measurement).  A flipped sign of
the pair (i, j) at scale k also moves G1 by up to (2 alpha / M_k) |p_i - p_j| (G0 not at all: the two terms cancel),
which reaches every pixel of the image through G1 ds/dp: that much, summed over the image's near-tie pairs and
multiplied by |ds/dp|, is granted as absolute slack.  The loss value takes no exemption (|e| is continuous), `dyadic`
none at all.  Worst exempt share over the case list: uniform 0.155 %, gauss 0 %, depth 0.619 %; `narrow`
would have 21 % and therefore runs with alpha = 0 only (it tests the conditioning, not the signs).

The only fixed constants: k = max(16, 4 k_ref) (k_from), the 2 % cap, the 16 2^-24 sign margin.

k.  Procedure (as in the other check modules): evaluate the same formulae in plain fp32 torch (`EVAL`: `sum()`
reductions and autograd, neither the library nor the engine), run it through these checks over the GPU module's case
list (`measure_k_ref`) on the CPU and on the MI355X, record the worst error / (2^-24 mag) per check, and set
k = max(16, 4 k_ref) rounded up to a power of two.  The kernels' column is what tests/test_gpu_loss_kernels.py
printed on an MI355X (its last test).

    check            k_ref CPU  k_ref MI355X  k     kernels' worst ratio
    ssi_loss             0.26         0.27    16     0.26
    ssi_dpred            1.02         0.63    16     0.88
    ssi_dyadic           0.00         0.00    16     0.00  (every element equal in value: also a `same` check)
    ssi_dyadic_loss      0.00         0.00    16     0.00
    ssi_admit            0.00         0.00    16     0.00
    dice_loss            0.35         0.30    16     1.25
    dice_dlogits         1.44         1.44    16     1.44
    nce_loss             0.40         0.40    16     0.40
    nce_dq               0.63         0.89    16     0.52
    ce_loss              1.20         1.64    16     1.17
    ce_dlogits           2.28         2.28    16     2.47
    softce_loss          1.14         1.09    16     0.98
    softce_dlogits       4.83         2.09    32     2.19
    bt_loss              0.43         1.56    16     0.43

Input families (generated on the CPU from fixed seeds; the SSI target is masked as in test_gpu_losses.py: a quarter of
the pixels 0, the top third of image 0 masked):
    ssi    uniform (rand / rand), gauss (randn / rand + 0.05), depth (t = 5 rand + 0.1, p = 0.3 t + 0.2 + 0.05 randn),
           narrow (p = 0.5 + 0.01 randn), dyadic, degenerate, perfect_fit
    dice   gauss (2 randn), saturated (30 randn: the sigmoid is 0 or 1), empty (target 0, logits <= -20), full (target 1)
    ce     plain, scaled (x 30), neg_inf (-inf at a quarter of the non-target positions), each unweighted, weighted and
           `weight0` (the class of row 0 has weight 0)
    softce plain, scaled, one_hot_soft, mixup (targets that sum to 0.5 .. 1.5), and the label form at smoothing 0.1
    nce    test_gpu_loss_heads._nce_case's (positives that look like their queries, a key of norm 0), zero_query
    bt     corr (0.05 randn + 0.9 I), integers
"""
import math

import torch
import torch.nn.functional as Fn

import finetune_checks as fc
import map_checks as mc
from ln_checks import EPS32, F64, F32, k_from, u_of      # noqa: F401
from map_checks import _gen

BOUNDED = ("ssi_loss", "ssi_dpred", "ssi_dyadic", "ssi_dyadic_loss", "ssi_admit", "dice_loss", "dice_dlogits",
           "nce_loss", "nce_dq", "ce_loss", "ce_dlogits", "softce_loss", "softce_dlogits", "bt_loss")
EXACT = ("ssi_zero", "ssi_exempt", "ce_zero", "bt_exact")
CHECKS = BOUNDED
# worst error / (2^-24 mag) of the fp32 torch evaluation over the GPU module's case list (measure_k_ref)
K_REF_CPU = {"ssi_loss": 0.264, "ssi_dpred": 1.020, "ssi_dyadic": 0.0, "ssi_dyadic_loss": 0.0, "ssi_admit": 0.0,
             "dice_loss": 0.351, "dice_dlogits": 1.437, "nce_loss": 0.396, "nce_dq": 0.630, "ce_loss": 1.203,
             "ce_dlogits": 2.281, "softce_loss": 1.143, "softce_dlogits": 4.832, "bt_loss": 0.426}
K_REF_GPU = {"ssi_loss": 0.265, "ssi_dpred": 0.630, "ssi_dyadic": 0.0, "ssi_dyadic_loss": 0.0, "ssi_admit": 0.0,
             "dice_loss": 0.304, "dice_dlogits": 1.438, "nce_loss": 0.396, "nce_dq": 0.885, "ce_loss": 1.640,
             "ce_dlogits": 2.281, "softce_loss": 1.088, "softce_dlogits": 2.087, "bt_loss": 1.561}
# the kernels' worst ratio per check, as tests/test_gpu_loss_kernels.py printed it on an MI355X
KERNELS = {"ssi_loss": 0.26, "ssi_dpred": 0.88, "ssi_dyadic": 0.0, "ssi_dyadic_loss": 0.0, "ssi_admit": 0.0,
           "dice_loss": 1.25, "dice_dlogits": 1.44, "nce_loss": 0.40, "nce_dq": 0.52, "ce_loss": 1.17,
           "ce_dlogits": 2.47, "softce_loss": 0.98, "softce_dlogits": 2.19, "bt_loss": 0.43}
K_REF = {n: max(K_REF_CPU.get(n, 0.0), K_REF_GPU.get(n, 0.0)) for n in CHECKS}
K = {name: k_from(v) for name, v in K_REF.items()}
SENTINEL = 12288.0
SIGN_MARGIN = 16.0          # x 2^-24 (d(d_i) + d(d_j)): a pair difference this small has no sign to pin
EXEMPT_CAP = 0.02           # of a case's elements
TINY = 2.0 ** -102          # 2^-126 / 2^-24: a result below the smallest normal may arrive as 0
NCE_EPS = float(torch.tensor(1e-12, dtype=F32))
NB, CE_MAXBLK, BT_MAXBLK = 32, 512, 1024        # loss_ops.hip
NCE_TR, NCE_TK, NCE_MAXCHUNK = 32, 64, 64


def f32(v):
    """the Python float rounded to fp32, as the C ABI hands it over"""
    return float(torch.tensor(v, dtype=F32))


def nce_plan(N, M):
    """nce_plan of loss_ops.hip: (rowtiles, nsub, spc, nchunk)"""
    rowtiles, nsub = -(-N // NCE_TR), -(-M // NCE_TK)
    want = min(-(-512 // rowtiles), NCE_MAXCHUNK, nsub)
    spc = -(-nsub // want)
    return rowtiles, nsub, spc, -(-nsub // spc)


class Report(mc.Report):
    def __init__(self, tag="", measure=False, k=None):
        super().__init__(tag, measure, K if k is None else k)
        self.exempt = {}        # tag -> (exempt pixels, elements)
        self.bit_equal = {}     # check -> (bit-equal elements, elements)

    def count_equal(self, name, got, ref):
        a, b = self.bit_equal.get(name, (0, 0))
        want = ref.to(got.dtype).reshape(got.shape)
        self.bit_equal[name] = (a + int((got == want).sum()), b + got.numel())

    def zero(self, name, got, where, what):
        """got is +-0 at `where`"""
        z = torch.zeros_like(got)
        self.same(name, torch.where(where, got, z).abs(), z, what)
        if self.measure:
            self.worst.setdefault(name, 0.0)

    def merge(self, other):
        self.exempt.update(getattr(other, "exempt", {}))
        for n, (a, b) in getattr(other, "bit_equal", {}).items():
            a0, b0 = self.bit_equal.get(n, (0, 0))
            self.bit_equal[n] = (a0 + a, b0 + b)
        return super().merge(other)


def _dev(c):
    return c.get("device", "cpu")


def _t(c, name, dt=None):
    t = c[name]
    return None if t is None else t.to(device=_dev(c)) if dt is None else t.to(device=_dev(c), dtype=dt)


def _cpu(o):
    return {k: (v.detach().cpu() if torch.is_tensor(v) else v) for k, v in o.items()}


def _grad(loss, x):
    """d loss / d x, zeros where loss does not depend on x"""
    if not loss.requires_grad:
        return torch.zeros_like(x)
    g, = torch.autograd.grad(loss, x, allow_unused=True)
    return torch.zeros_like(x) if g is None else g


def _v(x):
    return x.view(-1, 1, 1)


# ===================================================================== ssi
SSI_FAMILIES = ("uniform", "gauss", "depth", "narrow", "dyadic", "degenerate", "perfect_fit")


def _masked(t, g):
    B, H, W = t.shape
    t = torch.where(torch.rand(B, H, W, generator=g) < 0.25, torch.zeros(()), t)
    t[0, : H // 3] = 0
    return t


def ssi_case(family, B, H, W, alpha, scales, seed=0):
    g = _gen(41, seed, SSI_FAMILIES.index(family), B, H, W, int(alpha * 8), scales)
    sh = (B, H, W)
    if family in ("uniform", "degenerate"):
        p, t = torch.rand(sh, generator=g), _masked(torch.rand(sh, generator=g), g)
    elif family == "gauss":
        p, t = torch.randn(sh, generator=g), _masked(torch.rand(sh, generator=g) + 0.05, g)
    elif family == "depth":
        t = 5 * torch.rand(sh, generator=g) + 0.1
        p, t = 0.3 * t + 0.2 + 0.05 * torch.randn(sh, generator=g), _masked(t, g)
    elif family == "narrow":
        p, t = 0.5 + 0.01 * torch.randn(sh, generator=g), _masked(torch.rand(sh, generator=g), g)
    elif family == "perfect_fit":
        p = torch.randint(0, 256, sh, generator=g).float() / 64
        t = _masked(2 * p + 1, g)
    elif family == "dyadic":
        assert sh == (3, 16, 16)
        t = torch.randint(1, 17, sh, generator=g).float() / 4
        t[1, :, :8] = 0
        t[2, :8, :] = 0
        p = torch.zeros(sh)
        for b in range(B):
            idx = (t[b] > 0).reshape(-1).nonzero().reshape(-1)
            idx = idx[torch.randperm(idx.numel(), generator=g)]
            v = torch.ones(idx.numel())
            v[: idx.numel() // 2] = -1
            p[b].view(-1)[idx] = v
    if family == "degenerate":
        assert B >= 4 and H >= 10 and W >= 10
        t[1] = 0                                            # no valid pixel
        t[2] = 0
        t[2, 5, 7] = 0.75                                   # one valid pixel
        t[3] = 0
        t[3, 8, 8], t[3, 8, 9] = 0.5, 0.875                 # two valid pixels of equal prediction, neighbours
        p[3, 8, 9] = p[3, 8, 8]
    return {"kind": "ssi", "family": family, "shape": sh, "alpha": float(alpha), "scales": scales,
            "pred": p.contiguous(), "target": t.contiguous()}


def _bb(total, div):
    """_batch_based of losses.py"""
    return torch.where(div == 0, torch.zeros_like(total), total / torch.clamp(div, min=1e-30))


def _abs_sign0_is_1(e):
    return torch.where(e >= 0, e, -e)


def ssi_scale_shift(p, t, m):
    a00, a01, a11 = (m * p * p).sum((1, 2)), (m * p).sum((1, 2)), m.sum((1, 2))
    b0, b1 = (m * p * t).sum((1, 2)), (m * t).sum((1, 2))
    det = a00 * a11 - a01 * a01
    ok = det != 0
    safe = torch.where(ok, det, torch.ones_like(det))
    s = torch.where(ok, (a11 * b0 - a01 * b1) / safe, torch.zeros_like(det))
    h = torch.where(ok, (-a01 * b0 + a00 * b1) / safe, torch.zeros_like(det))
    return s, h, ok


def ssi_formula(p, t, alpha, scales, mut=None):
    """the loss of ScaleAndShiftInvariantLoss (batch-based) in the dtype of p"""
    m = (t > 0).to(p.dtype)
    s, h, ok = ssi_scale_shift(p, t, m)
    if mut == "ssi_scale_shift_constant":
        s, h = s.detach(), h.detach()
    if mut == "ssi_singular_gets_scale":
        s = torch.where(ok, s, torch.ones_like(s))
    ssi = _v(s) * p + _v(h)
    M0 = m.sum()
    res = ssi - t
    loss = _bb((m * res * res).sum(), (1.0 if mut == "ssi_mse_over_M" else 2.0) * M0)
    if alpha > 0:
        ab = _abs_sign0_is_1 if mut == "ssi_sign0_is_1" else torch.abs
        d0 = m * (ssi - t)
        H, W = p.shape[1:]
        for k in range(scales):
            st = 2 ** k
            mk, dk = m[:, ::st, ::st], d0[:, ::st, ::st]
            Mk = M0 if mut == "ssi_scale_k_over_M0" else mk.sum()
            if mut == "ssi_fine_neighbours" and st > 1:         # the pixel next door, not the next of the grid
                ax, bx = d0[:, ::st, :W - 1][:, :, ::st], d0[:, ::st, 1:][:, :, ::st]
                wx = m[:, ::st, :W - 1][:, :, ::st] * m[:, ::st, 1:][:, :, ::st]
                ay, by = d0[:, :H - 1, ::st][:, ::st], d0[:, 1:, ::st][:, ::st]
                wy = m[:, :H - 1, ::st][:, ::st] * m[:, 1:, ::st][:, ::st]
            else:
                ax, bx, ay, by = dk[:, :, :-1], dk[:, :, 1:], dk[:, :-1], dk[:, 1:]
                wx, wy = mk[:, :, 1:] * mk[:, :, :-1], mk[:, 1:] * mk[:, :-1]
                if mut == "ssi_pair_one_mask":
                    wx, wy = mk[:, :, :-1], mk[:, :-1]
            loss = loss + alpha * _bb((ab(bx - ax) * wx).sum() + (ab(by - ay) * wy).sum(), Mk)
    return loss


def ssi_ref(c):
    """fp64: loss, dpred (autograd), the closed form and every mag of the ssi checks"""
    if "_ref" in c:
        return c["_ref"]
    p, t = c["pred"].to(F64), c["target"].to(F64)
    alpha, scales = f32(c["alpha"]), c["scales"]
    pr = p.clone().requires_grad_(True)
    loss = ssi_formula(pr, t, alpha, scales)
    grad = _grad(loss, pr)
    m = (t > 0).to(F64)
    n, a00, a01 = m.sum((1, 2)), (m * p * p).sum((1, 2)), (m * p).sum((1, 2))
    b0, b1 = (m * p * t).sum((1, 2)), (m * t).sum((1, 2))
    S1, Sb0 = (m * p.abs()).sum((1, 2)), (m * (p * t).abs()).sum((1, 2))
    det = a00 * n - a01 * a01
    ok = det != 0
    okf = ok.to(F64)
    safe = torch.where(ok, det, torch.ones_like(det))
    s, h = okf * (n * b0 - a01 * b1) / safe, okf * (a00 * b1 - a01 * b0) / safe
    ddet = 2 * a00 * n + 2 * S1 * S1
    d_s = okf * ((2 * n * Sb0 + 3 * S1 * b1 + s.abs() * ddet) / safe.abs() + s.abs())
    d_h = okf * ((3 * S1 * Sb0 + 3 * a00 * b1 + h.abs() * ddet) / safe.abs() + h.abs())
    d = m * (_v(s) * p + _v(h) - t)
    dd = m * (p.abs() * _v(d_s) + _v(d_h) + (_v(s) * p).abs() + _v(h).abs() + t.abs())
    M0 = float(m.sum())
    inv0 = 1.0 / M0 if M0 > 0 else 0.0
    g, mag_g, gmax = d * inv0, (d.abs() + dd) * inv0, d.abs() * inv0
    val, mag_val = float((d * d).sum()) * inv0 / 2, float((d * d + 2 * d.abs() * dd).sum()) * inv0 / 2
    exempt = torch.zeros_like(m, dtype=torch.bool)
    tie_g1 = torch.zeros_like(n)
    zero_pairs = 0
    for k in range(scales if alpha > 0 else 0):
        st = 2 ** k
        mk, dk, ddk, pk = m[:, ::st, ::st], d[:, ::st, ::st], dd[:, ::st, ::st], p[:, ::st, ::st]
        Mk = float(mk.sum())
        if Mk == 0:
            continue
        acc, cnt, ex = torch.zeros_like(dk), torch.zeros_like(dk), torch.zeros_like(dk, dtype=torch.bool)
        for lo, hi in (((slice(None), slice(None), slice(None, -1)), (slice(None), slice(None), slice(1, None))),
                       ((slice(None), slice(None, -1)), (slice(None), slice(1, None)))):
            w = mk[lo] * mk[hi]
            e = dk[hi] - dk[lo]
            sg = torch.sign(e) * w
            acc[hi] += sg
            acc[lo] -= sg
            cnt[hi] += w
            cnt[lo] += w
            near = (w > 0) & (e.abs() <= SIGN_MARGIN * EPS32 * (ddk[hi] + ddk[lo]))
            ex[hi] |= near
            ex[lo] |= near
            zero_pairs += int(((w > 0) & (e == 0)).sum())
            tie_g1 += (near.to(F64) * (pk[hi] - pk[lo]).abs()).sum((1, 2)) * (2 * alpha / Mk)
            val += alpha * float((e.abs() * w).sum()) / Mk
            mag_val += alpha * float(((e.abs() + ddk[hi] + ddk[lo]) * w).sum()) / Mk
        g[:, ::st, ::st] += alpha * acc / Mk
        mag_g[:, ::st, ::st] += alpha * cnt / Mk
        gmax[:, ::st, ::st] += alpha * cnt / Mk
        exempt[:, ::st, ::st] |= ex
    sm = lambda x: x.sum((1, 2))
    G0, G1, mG0, mG1 = sm(g), sm(g * p), sm(mag_g), sm(mag_g * p.abs())
    ddp, mdd = 2 * _v(n) * p - 2 * _v(a01), 2 * _v(n) * p.abs() + 2 * _v(S1)
    mo = m * _v(okf)
    dsdp = mo * (_v(n) * t - _v(b1) - _v(s) * ddp) / _v(safe)
    dhdp = mo * (2 * p * _v(b1) - _v(b0) - _v(a01) * t - _v(h) * ddp) / _v(safe)
    mag_ds = mo * ((_v(n) * t + _v(b1) + _v(s).abs() * mdd + _v(d_s) * ddp.abs() + dsdp.abs() * _v(ddet))
                   / _v(safe).abs() + dsdp.abs())
    mag_dh = mo * ((2 * p.abs() * _v(b1) + _v(Sb0) + _v(S1) * t + _v(h).abs() * mdd + _v(d_h) * ddp.abs()
                    + dhdp.abs() * _v(ddet)) / _v(safe).abs() + dhdp.abs())
    closed = g * _v(s) + _v(G1) * dsdp + _v(G0) * dhdp
    mag = (mag_g * _v(s).abs() + g.abs() * _v(d_s) + _v(mG1) * dsdp.abs() + _v(G1).abs() * mag_ds
           + _v(mG0) * dhdp.abs() + _v(G0).abs() * mag_dh)
    r = {"loss": loss.detach(), "dpred": grad, "closed": closed, "closed_loss": val, "mag_loss": torch.tensor(mag_val, dtype=F64),
         "mag": mag, "slack": _v(tie_g1) * dsdp.abs(), "exempt": exempt, "zero_pairs": zero_pairs,
         "mag_dyadic": (g * _v(s)).abs() + (_v(G1) * dsdp).abs() + (_v(G0) * dhdp).abs(),
         "admit": gmax * _v(s).abs() + _v(sm(gmax * p.abs())) * dsdp.abs() + _v(sm(gmax)) * dhdp.abs(),
         "singular": (~ok)[:, None, None].expand_as(p), "det": det, "scale": s, "shift": h}
    c["_ref"] = r
    return r


def ssi_eval(c, mut=None, dt=F32):
    p = _t(c, "pred", dt).clone().requires_grad_(True)
    loss = ssi_formula(p, _t(c, "target", dt), c["alpha"], c["scales"], mut)
    d = _grad(loss, p).clone()
    if mut == "ssi_image_scaled":
        d[0] *= 1 + 2.0 ** -10
    if mut == "ssi_element_off":
        r = ssi_ref(c)
        ok = ((r["mag"] > 0) & ~r["exempt"]).reshape(-1).nonzero().reshape(-1)
        if ok.numel():
            i = int(ok[ok.numel() // 2])
            d.view(-1)[i] += 2.0 ** -12 * float(r["mag"].reshape(-1)[i])
    return _cpu({"loss": loss.detach().float(), "dpred": d.float()})


def ssi_check(c, o, rep):
    r = ssi_ref(c)
    got = o["dpred"]
    if c["family"] == "dyadic":
        rep.bounded("ssi_dyadic_loss", o["loss"], r["loss"], r["loss"].abs())
        rep.bounded("ssi_dyadic", got, r["dpred"], r["mag_dyadic"])
        rep.same("ssi_dyadic", got + 0.0, r["dpred"].float() + 0.0, "not the exact value (zeros of either sign alike)")
        rep.count_equal("ssi_dyadic", got, r["dpred"])
        rep.count_equal("ssi_dyadic_loss", o["loss"], r["loss"])
    rep.bounded("ssi_loss", o["loss"], r["loss"], r["mag_loss"])
    rep.zero("ssi_zero", got, r["singular"], "dpred is not 0 on an image with a singular system")
    if c["family"] == "dyadic":         # no exemption at all
        return
    if c["family"] == "perfect_fit":
        fin = torch.isfinite(got)
        excess = torch.where(fin, (got.to(F64).abs() - r["admit"]).clamp_min(0), torch.full_like(r["admit"], math.inf))
        rep.bounded("ssi_admit", excess.float(), torch.zeros_like(r["admit"]), r["mag"])
        return
    ex = r["exempt"]
    n_ex, total = int(ex.sum()), ex.numel()
    rep.exempt[rep.tag] = (n_ex, total)
    rep.worst.setdefault("ssi_exempt", 0.0)
    if n_ex > EXEMPT_CAP * total and not rep.measure:
        rep.worst["ssi_exempt"] = math.inf
        rep.failed.append("%s ssi_exempt: %d of %d pixels exempt, more than %g" % (rep.tag, n_ex, total, EXEMPT_CAP))
    got = torch.where(ex, r["dpred"].to(got.dtype), got)
    rep.bounded("ssi_dpred", got, r["dpred"], r["mag"], slack=r["slack"])


# ===================================================================== dice
DICE_FAMILIES = ("gauss", "saturated", "empty", "full")
DICE_SMOOTH = 1e-8


def dice_case(family, B, n, seed=0):
    g = _gen(42, seed, DICE_FAMILIES.index(family), B, n)
    l = torch.randn(B, n, generator=g) * (30 if family == "saturated" else 2)
    t = (torch.rand(B, n, generator=g) < 0.3).float()
    if family == "empty":
        l, t = -20 - l.abs(), torch.zeros(B, n)
    if family == "full":
        t = torch.ones(B, n)
    return {"kind": "dice", "family": family, "shape": (B, n), "logits": l.contiguous(), "target": t}


def dice_formula(l, t, smooth, mut=None):
    B = l.shape[0]
    m1 = torch.sigmoid(l)
    sm = 0.0 if mut == "dice_no_smooth" else smooth
    score = 2.0 * ((m1 * t).sum(1) + sm) / ((m1 * m1).sum(1) + (t * t).sum(1) + sm)
    return 1 - score.sum() / (B + 1 if mut == "dice_wrong_B" else B)


def dice_ref(c):
    if "_ref" in c:
        return c["_ref"]
    l, t, sm = c["logits"].to(F64), c["target"].to(F64), f32(DICE_SMOOTH)
    B = l.shape[0]
    lr = l.clone().requires_grad_(True)
    loss = dice_formula(lr, t, sm)
    grad = _grad(loss, lr)
    m1 = torch.sigmoid(l)
    w = m1 * (1 - m1)
    dm1 = w * l.abs() + m1 + TINY
    num, den = (m1 * t).sum(1, keepdim=True) + sm, (m1 * m1).sum(1, keepdim=True) + (t * t).sum(1, keepdim=True) + sm
    dnum = ((m1 + dm1) * t.abs()).sum(1, keepdim=True) + sm
    dden = (m1 * m1 + 2 * m1 * dm1).sum(1, keepdim=True) + (t * t).sum(1, keepdim=True) + sm
    score = 2 * num / den
    mag_loss = 1 + (2 * (dnum / den + num * dden / den ** 2) + score.abs()).sum() / B
    ds = 2 * t / den - 4 * num * m1 / den ** 2
    mag_ds = ((2 * t / den).abs() + (4 * num * m1 / den ** 2).abs() + 2 * t.abs() * dden / den ** 2
              + 4 * (dnum * m1 + num * dm1) / den ** 2 + 8 * num * m1 * dden / den ** 3)
    r = {"loss": loss.detach(), "dlogits": grad, "closed": -(ds / B) * w, "mag_loss": mag_loss,
         "mag": (mag_ds * w + ds.abs() * (dm1 + w)) / B}
    c["_ref"] = r
    return r


def dice_eval(c, mut=None, dt=F32):
    l, t = _t(c, "logits", dt).clone().requires_grad_(True), _t(c, "target", dt)
    loss = dice_formula(l, t, DICE_SMOOTH, mut)
    d = _grad(loss, l)
    if mut == "dice_no_second_term":
        m1 = torch.sigmoid(l.detach())
        den = (m1 * m1).sum(1, keepdim=True) + (t * t).sum(1, keepdim=True) + DICE_SMOOTH
        d = -(2 * t / den / l.shape[0]) * m1 * (1 - m1)
    return _cpu({"loss": loss.detach().float(), "dlogits": d.float()})


def dice_check(c, o, rep):
    r = dice_ref(c)
    rep.bounded("dice_loss", o["loss"], r["loss"], r["mag_loss"])
    rep.bounded("dice_dlogits", o["dlogits"], r["dlogits"], r["mag"] + TINY)


# ===================================================================== infonce
NCE_FAMILIES = ("plain", "alike", "zero_query")


def nce_case(family, N, M, C, off, T, seed=0):
    """plain / alike: the inputs of test_gpu_loss_heads._nce_case (odd / even index there)"""
    g = _gen(43, seed, NCE_FAMILIES.index(family), N, M, C, off, int(T * 1000))
    q, k = torch.randn(N, C, generator=g), torch.randn(M, C, generator=g)
    if family == "alike":
        k[off:off + N] += 0.5 * q
    if off > 0:
        k[0] = 0                        # a key of norm 0, never a positive
    if family == "zero_query":
        q[N // 2] = 0
    return {"kind": "nce", "family": family, "shape": (N, M, C), "off": off, "T": float(T), "q": q, "k": k}


def nce_formula(q, k, T, off, mut=None):
    N = q.shape[0]
    qn, kn = Fn.normalize(q, dim=1, eps=NCE_EPS), Fn.normalize(k, dim=1, eps=NCE_EPS)
    logits = qn @ kn.t() / T
    labels = torch.arange(N, device=q.device) + (0 if mut == "nce_labels_without_offset" else off)
    scale = T if mut == "nce_T_for_2T" else 2 * T
    if mut == "nce_merge_without_rescale":      # per 64-key chunk (max, sum exp), merged without exp(m_old - m_new)
        ms, ss = [], []
        for j in range(0, logits.shape[1], NCE_TK):
            mj = logits[:, j:j + NCE_TK].max(1).values
            ms.append(mj)
            ss.append(torch.exp(logits[:, j:j + NCE_TK] - mj[:, None]).sum(1))
        lse = torch.stack(ms).max(0).values + torch.log(torch.stack(ss).sum(0))
        return (lse - logits[torch.arange(N), labels]).mean() * scale
    return Fn.cross_entropy(logits, labels) * scale


def nce_ref(c):
    if "_ref" in c:
        return c["_ref"]
    q, k, T, off = c["q"].to(F64), c["k"].to(F64), f32(c["T"]), c["off"]
    N = q.shape[0]
    qr = q.clone().requires_grad_(True)
    loss = nce_formula(qr, k, T, off)
    grad = _grad(loss, qr)
    qn, kn = Fn.normalize(q, dim=1, eps=NCE_EPS), Fn.normalize(k, dim=1, eps=NCE_EPS)
    l = qn @ kn.t() / T
    ar, lab = torch.arange(N), torch.arange(N) + off
    dl = (6.0 / T) * (qn.abs() @ kn.abs().t())
    lse = torch.logsumexp(l, 1)
    p = torch.exp(l - lse[:, None])
    dlse = (p * dl).sum(1) + l.max(1).values.abs() + 1
    mag_loss = (2 * T / N) * (dlse + dl[ar, lab] + lse.abs() + l[ar, lab].abs()).sum()
    dp = p * (dl + dlse[:, None] + (l - lse[:, None]).abs() + 1) + TINY
    pm = p.clone()
    pm[ar, lab] -= 1
    g = (2.0 / N) * (pm @ kn)
    mag_g = (2.0 / N) * ((3 * pm.abs() + dp) @ kn.abs())
    nrm = q.norm(dim=1, keepdim=True)
    big = nrm > NCE_EPS
    sn = torch.where(big, nrm, torch.ones_like(nrm))
    dot = (qn * g).sum(1, keepdim=True)
    dotmag = (qn.abs() * (mag_g + 2 * g.abs())).sum(1, keepdim=True)
    closed = torch.where(big, (g - qn * dot) / sn, g / NCE_EPS)
    mag = torch.where(big, (mag_g + qn.abs() * dotmag + 2 * (qn * dot).abs()) / sn + 2 * closed.abs(),
                      mag_g / NCE_EPS + closed.abs())
    r = {"loss": loss.detach(), "dq": grad, "closed": closed, "mag_loss": mag_loss, "mag": mag}
    c["_ref"] = r
    return r


def nce_eval(c, mut=None, dt=F32):
    q, k = _t(c, "q", dt).clone().requires_grad_(True), _t(c, "k", dt)
    loss = nce_formula(q, k, c["T"], c["off"], mut)
    d = _grad(loss, q).clone()
    if mut == "nce_zero_query_by_norm":
        z = (q.detach().norm(dim=1) == 0)
        d[z] = d[z] * NCE_EPS / q.detach().norm(dim=1)[z, None]
    return _cpu({"loss": loss.detach().float(), "dq": d.float()})


def nce_check(c, o, rep):
    r = nce_ref(c)
    rep.bounded("nce_loss", o["loss"], r["loss"], r["mag_loss"])
    rep.bounded("nce_dq", o["dq"], r["dq"], r["mag"] + TINY)


# ===================================================================== cross-entropy
CE_FAMILIES = ("plain", "scaled", "neg_inf")
CE_WEIGHTS = ("none", "weighted", "weight0")
CE_TRIP = 4 * CE_MAXBLK         # rows one sweep of the grid covers


def ce_case(family, weights, B, C, seed=0):
    g = _gen(44, seed, CE_FAMILIES.index(family), CE_WEIGHTS.index(weights), B, C)
    x = torch.randn(B, C, generator=g) * (30 if family == "scaled" else 1)
    t = torch.randint(0, C, (B,), generator=g)
    if B > 1 and C > 1:
        t[1] = (t[0] + 1) % C           # two classes present: the weight of one may be 0
    if family == "neg_inf" and C > 1:
        hole = torch.rand(B, C, generator=g) < 0.25
        hole[torch.arange(B), t] = False
        x = torch.where(hole, torch.tensor(-math.inf), x)
    w = None
    if weights != "none":
        w = torch.rand(C, generator=g) + 0.1
        if weights == "weight0" and B > 1 and C > 1:
            w[t[0]] = 0
    return {"kind": "ce", "family": family, "weights": weights, "shape": (B, C), "x": x.contiguous(), "t": t, "w": w}


def ce_formula(x, t, w, mut=None):
    B = x.shape[0]
    ar = torch.arange(B, device=x.device)
    nll = torch.logsumexp(x, 1) - x[ar, t]
    cls = x.argmax(1) if mut == "ce_weight_at_argmax" else t
    wt = torch.ones_like(nll) if w is None else w[cls]
    return (wt * nll).sum() / (B if mut == "ce_over_B" else wt.sum())


def ce_ref(c):
    if "_ref" in c:
        return c["_ref"]
    x, t = c["x"].to(F64), c["t"]
    w = None if c["w"] is None else c["w"].to(F64)
    B, C = x.shape
    xr = x.clone().requires_grad_(True)
    loss = Fn.cross_entropy(xr, t, weight=w)
    grad = _grad(loss, xr)
    ar = torch.arange(B)
    m, lse = x.max(1).values, torch.logsumexp(x, 1)
    sm = torch.exp(x - lse[:, None])
    wt = torch.ones(B, dtype=F64) if w is None else w[t]
    W = wt.sum()
    dlse = m.abs() + 1
    hot = Fn.one_hot(t, C).to(F64)
    arg = torch.where(sm > 0, (x - lse[:, None]).abs() + dlse[:, None], torch.zeros_like(x))
    r = {"loss": loss.detach(), "dlogits": grad, "mag_loss": (wt * (lse.abs() + x[ar, t].abs() + dlse)).sum() / W,
         "mag": wt[:, None] * (sm + hot + sm * arg + TINY) / W,
         "zero": ((wt == 0)[:, None] | (torch.isinf(x) & (hot == 0))).expand_as(x)}
    c["_ref"] = r
    return r


def ce_eval(c, mut=None, dt=F32):
    x, w = _t(c, "x", dt).clone().requires_grad_(True), _t(c, "w", dt)
    loss = ce_formula(x, _t(c, "t"), w, mut)
    d = _grad(loss, x).clone()
    if mut == "ce_second_trip_row_zeroed" and x.shape[0] > CE_TRIP:
        d[CE_TRIP] = 0
    return _cpu({"loss": loss.detach().float(), "dlogits": d.float()})


def ce_check(c, o, rep):
    r = ce_ref(c)
    rep.bounded("ce_loss", o["loss"], r["loss"], r["mag_loss"])
    rep.bounded("ce_dlogits", o["dlogits"], r["dlogits"], r["mag"] + TINY)
    rep.zero("ce_zero", o["dlogits"], r["zero"], "dlogits is not 0 in a weight-0 row or at a -inf logit")
    if not rep.measure and not bool(torch.isfinite(o["loss"])):
        rep.failed.append("%s ce_zero: the loss is not finite" % rep.tag)


# ===================================================================== soft-target / label-smoothing cross-entropy
SOFTCE_FAMILIES = ("plain", "scaled", "one_hot_soft", "mixup")
SMOOTHING = 0.1


def softce_case(family, form, B, C, seed=0):
    """form 'soft': targets [B, C] given; 'label': int64 labels and SMOOTHING"""
    g = _gen(45, seed, SOFTCE_FAMILIES.index(family), form == "label", B, C)
    x = torch.randn(B, C, generator=g) * (30 if family == "scaled" else 1)
    y = torch.randint(0, C, (B,), generator=g)
    t = None
    if form == "soft":
        if family == "one_hot_soft":
            t = Fn.one_hot(y, C).float()
        elif family == "mixup":
            lam = torch.rand(B, 1, generator=g)
            y2 = torch.randint(0, C, (B,), generator=g)
            t = lam * Fn.one_hot(y, C).float() + (1 - lam) * Fn.one_hot(y2, C).float()
            t = (0.9 * t + 0.1 / C) * (0.5 + torch.rand(B, 1, generator=g))
        else:
            t = torch.softmax(2 * torch.randn(B, C, generator=g), 1)
    return {"kind": "softce", "family": family, "form": form, "shape": (B, C), "x": x.contiguous(),
            "t": None if t is None else t.contiguous(), "y": y if form == "label" else None}


def softce_ref(c):
    if "_ref" in c:
        return c["_ref"]
    x = c["x"].to(F64)
    B, C = x.shape
    xr = x.clone().requires_grad_(True)
    if c["form"] == "soft":
        t = c["t"].to(F64)
        loss, T = fc.soft_target_ce(xr, t), t.abs()
    else:
        t = (1.0 - SMOOTHING) * Fn.one_hot(c["y"], C).to(F64) + SMOOTHING / C
        loss, T = fc.label_smoothing_ce(xr, c["y"], SMOOTHING), 4 * t.abs()
    grad = _grad(loss, xr)
    M = x.max(1, keepdim=True).values
    logs = torch.log(torch.exp(x - M).sum(1, keepdim=True))
    sm = torch.exp(x - M - logs)
    dlse = M.abs() + 1
    Ts, ts = T.sum(1, keepdim=True), t.abs().sum(1, keepdim=True)
    r = {"loss": loss.detach(), "dlogits": grad,
         "mag_loss": ((T * (logs.abs() + (x - M).abs())).sum(1, keepdim=True) + dlse * Ts).sum() / B,
         "mag": (sm * Ts + T + (sm * ((x - M - logs).abs() + dlse) + TINY) * ts) / B}
    c["_ref"] = r
    return r


def softce_eval(c, mut=None, dt=F32):
    x = _t(c, "x", dt).clone().requires_grad_(True)
    B, C = x.shape
    if c["form"] == "soft":
        t = _t(c, "t", dt)
        loss = fc.soft_target_ce(x, t)
        d = _grad(loss, x)
        if mut == "softce_sum_t_is_1":
            d = (torch.softmax(x.detach(), 1) - t) / B
    else:
        y = _t(c, "y")
        if mut == "softce_off_left_out":
            loss = ((1.0 - SMOOTHING) * (torch.logsumexp(x, 1) - x[torch.arange(B, device=x.device), y])).mean()
        else:
            loss = fc.label_smoothing_ce(x, y, SMOOTHING)
        d = _grad(loss, x)
    return _cpu({"loss": loss.detach().float(), "dlogits": d.float()})


def softce_check(c, o, rep):
    r = softce_ref(c)
    rep.bounded("softce_loss", o["loss"], r["loss"], r["mag_loss"])
    rep.bounded("softce_dlogits", o["dlogits"], r["dlogits"], r["mag"] + TINY)


# ===================================================================== Barlow Twins loss
BT_FAMILIES = ("corr", "integers")
LAMBD = 0.0051


def bt_case(family, D, seed=0):
    g = _gen(46, seed, BT_FAMILIES.index(family), D)
    if family == "integers":
        c = torch.randint(-16, 17, (D, D), generator=g).float() / 8
    else:
        c = 0.05 * torch.randn(D, D, generator=g) + 0.9 * torch.eye(D)
    return {"kind": "bt", "family": family, "shape": (D,), "c": c.contiguous()}


def bt_formula(c, lambd, mut=None, direct=False):
    D = c.shape[0]
    diag = torch.diagonal(c)
    on = (diag - 1).pow(2).sum()
    if mut == "bt_rows_beyond_1024_skipped":
        c, diag = c[:BT_MAXBLK], diag[:BT_MAXBLK]
        on = (diag - 1).pow(2).sum()
    if mut == "bt_diagonal_in_off_sum":
        return on + lambd * c.pow(2).sum()
    if direct:      # the off-diagonal terms summed directly, as the kernel does
        off = (c.pow(2) * (1 - torch.eye(c.shape[0], D, dtype=c.dtype, device=c.device))).sum()
    else:
        off = c.pow(2).sum() - diag.pow(2).sum()
    return on + lambd * off


def bt_ref(c):
    if "_ref" in c:
        return c["_ref"]
    x, lam = c["c"].to(F64), f32(LAMBD)
    diag = torch.diagonal(x)
    on, sq = (diag - 1).pow(2).sum(), x.pow(2).sum()
    off = sq - diag.pow(2).sum()
    exact = c["family"] == "integers" and float(sq) * 64 < 2 ** 24 and float(on) * 64 < 2 ** 24
    r = {"loss": bt_formula(x, lam), "mag": on + lam * off, "exact": exact}
    c["_ref"] = r
    return r


def bt_eval(c, mut=None, dt=F32):
    return _cpu({"loss": bt_formula(_t(c, "c", dt), LAMBD, mut, direct=True).float()})


def bt_check(c, o, rep):
    r = bt_ref(c)
    rep.bounded("bt_loss", o["loss"], r["loss"], r["mag"])
    rep.worst.setdefault("bt_exact", 0.0)
    if r["exact"]:
        rep.same("bt_exact", o["loss"], r["loss"].float(), "not the fp64 value rounded once")


# ===================================================================== table
KINDS = {"ssi": (ssi_case, ssi_eval, ssi_check), "dice": (dice_case, dice_eval, dice_check),
         "nce": (nce_case, nce_eval, nce_check), "ce": (ce_case, ce_eval, ce_check),
         "softce": (softce_case, softce_eval, softce_check), "bt": (bt_case, bt_eval, bt_check)}
EVAL = {kind: v[1] for kind, v in KINDS.items()}
# deliberately wrong fp32 evaluations: name -> (kind, the check that must catch it)
MUTATIONS = {
    "ssi_scale_shift_constant": ("ssi", "ssi_dpred"),       # no G0 / G1 terms
    "ssi_scale_k_over_M0": ("ssi", "ssi_loss"),             # M_0 as the divisor of scale k
    "ssi_fine_neighbours": ("ssi", "ssi_loss"),             # neighbours at distance 1 on the coarse grids
    "ssi_pair_one_mask": ("ssi", "ssi_loss"),               # a pair masked by one pixel's mask only
    "ssi_sign0_is_1": ("ssi", "ssi_dyadic"),
    "ssi_mse_over_M": ("ssi", "ssi_loss"),                  # M for 2M
    "ssi_image_scaled": ("ssi", "ssi_dyadic"),              # image 0's gradient times 1 + 2^-10
    "ssi_element_off": ("ssi", "ssi_dpred"),                # one element off by 2^-12 of its mag
    "ssi_singular_gets_scale": ("ssi", "ssi_zero"),         # a singular image with scale 1
    "dice_no_smooth": ("dice", "dice_loss"),
    "dice_no_second_term": ("dice", "dice_dlogits"),
    "dice_wrong_B": ("dice", "dice_loss"),                  # mean over B + 1
    "ce_over_B": ("ce", "ce_loss"),                         # B for sum w
    "ce_weight_at_argmax": ("ce", "ce_loss"),
    "ce_second_trip_row_zeroed": ("ce", "ce_dlogits"),      # row 2048, the first of the second grid-stride trip
    "softce_sum_t_is_1": ("softce", "softce_dlogits"),      # on `mixup`
    "softce_off_left_out": ("softce", "softce_loss"),
    "nce_labels_without_offset": ("nce", "nce_loss"),
    "nce_T_for_2T": ("nce", "nce_loss"),
    "nce_merge_without_rescale": ("nce", "nce_loss"),       # chunk sums added without exp(m_old - m_new)
    "nce_zero_query_by_norm": ("nce", "nce_dq"),
    "bt_diagonal_in_off_sum": ("bt", "bt_loss"),
    "bt_rows_beyond_1024_skipped": ("bt", "bt_loss"),
}


def make(kind, args):
    return KINDS[kind][0](*args)


def to_device(c, device):
    """the case with `device` noted: the fp32 evaluation moves what it needs, the references stay on the CPU"""
    return dict(c, device=device)


def tag_of(c):
    extra = {"ssi": lambda: "a%g s%d" % (c["alpha"], c["scales"]), "ce": lambda: c["weights"],
             "softce": lambda: c["form"], "nce": lambda: "off%d T%g" % (c["off"], c["T"])}.get(c["kind"], lambda: "")()
    return "%s %s %s %s" % (c["kind"], c["family"], c["shape"], extra)


def run_check(c, o, tag="", measure=False, k=None):
    rep = Report(tag or tag_of(c), measure, k)
    KINDS[c["kind"]][2](c, o, rep)
    return rep


def evaluate(c, mut=None):
    return KINDS[c["kind"]][1](c, mut if mut is not None and MUTATIONS[mut][0] == c["kind"] else None)


# ------------------------------------------------------------------ the case list of the GPU module
# ssi (B, H, W): H = W = 1; odd and below 8 (3 x 5: from scale 1 on the coarse grid is 2 x 3, 1 x 2, 1 x 1; 7 x 9:
# 1 x 2 at scale 3: grids with a single row); 17 x 19 odd; 33 x 40 two blocks per image; 96 x 96: HW = 9216 > 8192 =
# NB x 256, the second grid-stride trip of ssi_sums / ssi_grad; B = 300 > 256: the second trip of the finalize kernels
SSI_SMALL = ((2, 1, 1), (3, 3, 5), (2, 7, 9), (4, 17, 19))
SSI_ALPHAS = (0.0, 0.5, 1.0)
# dice (B, n): n = 8197 > 8192: the second trip of dice_sums; B = 300 > 256: the second trip of dice_finalize
DICE_SHAPES = ((1, 1), (1, 77), (3, 1000), (2, 8197), (300, 5))
# nce (N, M, C, off, T).  (8, 4200): one row tile, 66 sub-tiles, want = 64 -> spc = 2; (500, 2200): 16 row tiles,
# want = 32, 35 sub-tiles -> spc = 2; C = 1024: four features per thread of the finalize; C = 257, 30: ragged feature
# steps; T = 0.002: logits of +-500
NCE_SHAPES = ((1, 1, 1, 0, 1.0), (5, 7, 24, 2, 1.0), (17, 51, 257, 17, 0.2), (33, 99, 30, 66, 1.0),
              (8, 4200, 16, 100, 0.2), (500, 2200, 8, 1700, 0.2), (4, 70, 1024, 0, 0.2), (64, 128, 16, 64, 0.002))
NCE_SPC2 = ((8, 4200), (500, 2200))
NCE_ZERO_QUERY = (5, 7, 24, 2, 1.0)
# ce (B, C): C on either side of the 64 lanes; B = 2049 > 4 x 512 rows: the second grid-stride trip of both kernels
CE_SHAPES = ((1, 1), (5, 2), (7, 63), (7, 64), (7, 65), (130, 1000), (2049, 6))
# bt D: 1025 the scalar path, 1028 the ld4 path, both with rows 1024.. on the second trip of the row loop
BT_DIMS = (1, 129, 256, 1025, 1028)


def gpu_specs(kind):
    """(group, arguments of the kind's case constructor) of every case tests/test_gpu_loss_kernels.py runs"""
    out = []
    if kind == "ssi":
        fams = ("uniform", "gauss", "depth")
        for i, s in enumerate(SSI_SMALL):
            for scales in (1, 2, 3, 4):
                for j, a in enumerate(SSI_ALPHAS):
                    out.append(("%dx%dx%d" % s, (fams[(i + scales + j) % 3],) + s + (a, scales)))
            out.append(("%dx%dx%d" % s, ("narrow",) + s + (0.0, 4)))
        out.append(("degenerate", ("degenerate", 4, 17, 19, 0.5, 4)))
        out.append(("degenerate", ("degenerate", 4, 17, 19, 0.0, 1)))
        for scales in (1, 2, 3, 4):
            out.append(("dyadic", ("dyadic", 3, 16, 16, 0.5, scales)))
        for f, a in (("uniform", 0.5), ("gauss", 0.5), ("depth", 1.0), ("narrow", 0.0), ("perfect_fit", 0.5)):
            out.append(("2x33x40", (f, 2, 33, 40, a, 4)))
        for f, a in (("uniform", 0.5), ("depth", 1.0), ("narrow", 0.0), ("perfect_fit", 1.0)):
            out.append(("2x96x96", (f, 2, 96, 96, a, 4)))
        for f, a, sc in (("uniform", 0.5, 4), ("gauss", 0.0, 1), ("depth", 1.0, 2)):
            out.append(("300x3x5", (f, 300, 3, 5, a, sc)))
    elif kind == "dice":
        for s in DICE_SHAPES:
            for f in DICE_FAMILIES:
                out.append(("%dx%d" % s, (f,) + s))
    elif kind == "nce":
        for i, s in enumerate(NCE_SHAPES):
            out.append(("%dx%dx%d" % s[:3], (("alike", "plain")[i % 2],) + s))
        out.append(("zero_query", ("zero_query",) + NCE_ZERO_QUERY))
        out.append(("zero_query", ("zero_query", 33, 99, 30, 66, 1.0)))
    elif kind == "ce":
        for s in CE_SHAPES:
            for f in CE_FAMILIES:
                for w in CE_WEIGHTS:
                    out.append(("%dx%d" % s, (f, w) + s))
    elif kind == "softce":
        for s in CE_SHAPES:
            for f in SOFTCE_FAMILIES:
                out.append(("%dx%d" % s, (f, "soft") + s))
            for f in ("plain", "scaled"):
                out.append(("%dx%d" % s, (f, "label") + s))
    elif kind == "bt":
        for D in BT_DIMS:
            for f in BT_FAMILIES:
                out.append(("D%d" % D, (f, D)))
    return out


def groups(specs):
    return list(dict.fromkeys(s[0] for s in specs))


def measure_k_ref(device, log=print):
    """worst error / (2^-24 mag) per bounded check of the fp32 torch evaluation over the GPU module's case list"""
    worst = {}
    for kind in KINDS:
        for grp, a in gpu_specs(kind):
            c = to_device(make(kind, a), device)
            rep = run_check(c, evaluate(c), measure=True)
            for n, v in rep.worst.items():
                if n in BOUNDED and v > worst.get(n, -1.0):
                    worst[n] = v
                    log("k_ref %s = %.3f at %s %s %s" % (n, v, kind, grp, a[0]))
    return worst


def table(kernels=None):
    """the table of the docstring; `kernels`: worst ratio per check of the GPU module (default: the recorded one)"""
    kernels = KERNELS if kernels is None else kernels
    rows = ["    check            k_ref CPU  k_ref MI355X  k     kernels' worst ratio"]
    for n in BOUNDED:
        kr = "-" if n not in kernels else "%.2f" % kernels[n]
        if n == "ssi_dyadic":
            kr += "  (every element equal in value: also a `same` check)"
        rows.append("    %-16s %8.2f     %8.2f   %3d     %s" % (n, K_REF_CPU.get(n, float("nan")),
                                                               K_REF_GPU.get(n, float("nan")), K[n], kr))
    return "\n".join(rows)
