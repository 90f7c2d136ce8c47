"""fp64 references of the map and layout kernels (pooling, resampling, patch matrices, scatter / gather, pointwise
maps, the depth head, the momentum update) and the per-element checks that pin the kernels of dpt_ops.hip,
resnet_ops.hip and det_ops.hip to them (tests/test_gpu_map_kernels.py; proof that the checks bite:
tests/test_map_checks_cpu.py).

References: plain torch ops on the CPU in float64, starting from exactly what the kernel is handed (a bf16 input is
rounded first and the reference sees the rounded values; the pool backward starts from the arg bytes it is given, the
depth head backward from the y it is given).  Maps are channels-last, [B, H, W, C].
    bilinear2x        F.interpolate(scale_factor=2, mode="bilinear", align_corners=True) and its autograd
    maxpool3x3s2      F.max_pool2d(x, 3, 2, 1, return_indices=True), the flat index turned into dy * 3 + dx
    maxpool2x2        F.max_pool2d(x, 2), the gradient scattered to its indices
    avgpool           mean over H, W; dy / HW
    im2col3x3         F.unfold(act(x), 3, padding=1, stride), columns re-ordered to (dy, dx, c), zero up to ld
    col2im3x3         F.fold of dcols re-ordered from (dy, dx, c) to F.unfold's (c, dy, dx)
    pixel (un)shuffle, tokens <-> map, subsample2: written out by index (reshape / permute / slices)
    depth head        sigmoid(conv1x1(relu(x))); ds = dy y (1 - y), dx = [x > 0] ds w, dw = sum_m ds relu(x), db = sum_m ds
    gelu_map          F.gelu and its autograd;  ema_update: dst m + src (1 - m) with m as rounded to fp32
    stem_im2col7x7    F.unfold(img, 7, padding=3, stride=2) re-ordered to (dy, dx, c), zero from column 147

Two kinds of check, per output element, never a global norm.
  Bit for bit (`Report.same`: dtype, shape and the BITS, so that +0 and -0 differ): every output that is a copy, a
  cast, a selection, or one correctly rounded fp32 operation followed by at most one RNE rounding to bf16 —
  im2col (pad columns included), stem, sub_fwd / sub_bwd, unshuffle, shuffle (no bias), tok2map, map2tok, pool_y,
  pool_arg, pool2_y, pool2_dx, add, relu_bwd (the torch expression evaluated in the tensor's dtype); with the
  `integers` family also col2im, pool_dx, avg_fwd where HW is a power of two, shuffle_bias and ema at m in (0, 1)
  (`exact`: every sum, and the one division, is exact).
  Bounded: |got - ref| <= u |ref| + slack + k 2^-24 mag, u = 2^-8 for a bf16 output (its one final rounding) and 0
  otherwise, mag = the fp64 sum of the ABSOLUTE values of the terms the kernel adds:
    bl_fwd        sum over the four taps |w f|: every product and the three multiply-adds round at that size
    bl_bwd        sum over the contributing outputs |cy cx dy|
    pool_dx       sum |dy| routed to the pixel (up to four windows)
    col2im        sum |terms| (up to nine)
    avg_fwd       mean |x|: a running sum of HW terms, each add rounds at no more than the sum of |x| so far
    avg_bwd       |dy| / HW (one division)
    shuffle_bias  |g| + |bias|
    head_y        y (1 - y) (|b| + sum_c |relu(x) w|) + y: an error e of the pre-activation s (its sum, and the
                  exponent's argument, which the fast exponential rounds at the size of |s|) moves the sigmoid by
                  y (1 - y) e; 1 + exp(-s) and the reciprocal round at the size of y
    head_dx       |ds w|;   head_dw  sum_m |ds relu(x)|;   head_db  sum_m |ds|   (+ |initial| with accumulate)
    gelu_fwd      |x|: 0.5 x (1 + erf) cancels for x << 0 (1 + erf -> 0 with an absolute error of 2^-24), and torch's
                  fp32 kernel uses the same formula: the error is relative to x, not to gelu(x)
    gelu_bwd      |dy| (1 + |x| phi(x)): cdf <= 1 rounds at 1, x pdf at its own size
    ema           |dst m| + |src (1 - m)|
  slack (bilinear only): the kernels form the source coordinate in fp32, s = d fl((n - 1) / (2n - 1)): two roundings,
  |error of s| <= 2^-23 s, and the weight w1 = s - i0 (an exact subtraction) carries it.  In the forward an error e of
  wx moves the output by e |lerp_y(f[., x1] - f[., x0])|: slack = 2^-23 (sx Dx + sy Dy), Dx = sum_y wy |f[y, x1] -
  f[y, x0]| and Dy alike — coordinate times the difference of the two taps, charged outside k.  In the backward the
  two taps' weights of output o go to different pixels: slack = 2^-23 sum_o |dy[o]| (sx(o) [ix is a tap of o] cy +
  sy(o) [iy is a tap of o] cx).  The reference's taps of the last output are (n - 2, n - 1) with w1 = 1, the same value as
  (n - 1, n - 1), so that a coordinate that lands just below n - 1 is covered by the same term; every other
  coordinate is at least 1 / (2n - 1) away from an integer.

k.  Procedure (as in bn_checks / attn_checks / ln_checks): evaluate the same formulae in plain fp32 torch (`EVAL`,
neither the kernels nor the engine: fp32 coordinates and lerps, a running sum for the average pool, `sum()` for the
depth head), run it through these checks over the case list of the GPU module (`measure_k_ref`), record the worst
error / (2^-24 mag) per check as k_ref — the larger of torch on the CPU and torch on the MI355X — and set
k = max(16, 4 k_ref) rounded up to a power of two.

avg_fwd: the 14.9 is the `negative` family at HW = 196 — a running sum of 196 terms of one sign, whose partial sums
grow to the full sum (the bound of a running sum is (HW - 1) 2^-24 sum |x|); every other family stays below 3.  The
kernels' column is what tests/test_gpu_map_kernels.py printed on an MI355X (its last test).

    check         k_ref CPU  k_ref MI355X  k     kernels' worst ratio
    bl_fwd            2.14         2.14    16     1.34
    bl_bwd            0.73         0.73    16     1.13
    pool_dx           1.84         1.76    16     2.10
    col2im            2.82         2.82    16     2.82
    avg_fwd          14.94        14.94    64    14.9
    avg_bwd           0.98         1.33    16     0.98
    shuffle_bias      1.00         1.00    16     1.00
    head_y            1.89         1.85    16     2.48
    head_dx           3.55         3.55    16     3.55
    head_dw           1.98         1.68    16     1.82
    head_db           1.43         1.36    16     1.36
    gelu_fwd          1.70         1.83    16     1.83
    gelu_bwd          2.44         2.50    16     2.50
    ema               1.91         1.91    16     1.49

Input families (generated on the CPU from fixed seeds):
    gauss        N(0, 1)
    quarter      multiples of 1/4 in [-2, 2] through ReLU: many exact ties and zeros, the first-maximum rule decides
    negative     all below 0: a border window must not win with its padding (the pad is -inf, not 0)
    signed_zero  N(0, 1) with +0.0 and -0.0 at a quarter of the positions each (masks on x > 0; relu_raw clears signs)
    integers     in [-4, 4]: every sum is exact
"""
import math

import torch
import torch.nn.functional as Fn

import ln_checks as lc
from ln_checks import EPS32, F64, F32, BF, k_from, u_of      # noqa: F401

BOUNDED = ("bl_fwd", "bl_bwd", "pool_dx", "col2im", "avg_fwd", "avg_bwd", "shuffle_bias", "head_y", "head_dx",
           "head_dw", "head_db", "gelu_fwd", "gelu_bwd", "ema")
EXACT = ("im2col", "stem", "sub_fwd", "sub_bwd", "unshuffle", "shuffle", "tok2map", "map2tok", "pool_y", "pool_arg",
         "pool2_y", "pool2_dx", "add", "relu_bwd")
CHECKS = BOUNDED
# worst error / (2^-24 mag) of the fp32 torch evaluation over the GPU module's case list (measure_k_ref)
K_REF_CPU = {"bl_fwd": 2.143, "bl_bwd": 0.734, "pool_dx": 1.840, "col2im": 2.821, "avg_fwd": 14.944, "avg_bwd": 0.979,
             "shuffle_bias": 1.000, "head_y": 1.887, "head_dx": 3.551, "head_dw": 1.978, "head_db": 1.425,
             "gelu_fwd": 1.703, "gelu_bwd": 2.440, "ema": 1.911}
K_REF_GPU = {"bl_fwd": 2.143, "bl_bwd": 0.734, "pool_dx": 1.762, "col2im": 2.821, "avg_fwd": 14.944, "avg_bwd": 1.334,
             "shuffle_bias": 1.000, "head_y": 1.852, "head_dx": 3.551, "head_dw": 1.675, "head_db": 1.356,
             "gelu_fwd": 1.834, "gelu_bwd": 2.502, "ema": 1.911}
K_REF = {n: max(K_REF_CPU.get(n, 0.0), K_REF_GPU.get(n, 0.0)) for n in CHECKS}
K = {name: k_from(v) for name, v in K_REF.items()}
FAMILIES = ("gauss", "quarter", "negative", "signed_zero", "integers")
HEAD_GRID_ROWS = 1024 * 256          # rows one sweep of depth_head_bwd_kernel's grid covers


def V(dtype):
    """elements of a 16-byte chunk"""
    return 8 if dtype == BF else 4


def dname(dtype):
    return "bf16" if dtype == BF else "fp32"


class Report(lc.Report):
    def __init__(self, tag="", measure=False, k=None):
        super().__init__(K if k is None else k, tag, measure)

    def same(self, name, got, want, what="differs"):
        """dtype, shape and bits (+0 and -0 differ; no NaN is expected on either side)"""
        if self.measure:
            return
        self.worst.setdefault(name, 0.0)
        if got.dtype != want.dtype or got.shape != want.shape:
            self.worst[name] = math.inf
            self.failed.append("%s %s: %s: %s %s, want %s %s" % (self.tag, name, what, got.dtype, tuple(got.shape),
                                                                 want.dtype, tuple(want.shape)))
            return
        iv = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[got.element_size()]
        bad = (got.contiguous().view(iv) != want.contiguous().view(iv)).reshape(-1)
        if bool(bad.any()):
            i = int(bad.nonzero()[0])
            self.worst[name] = math.inf
            self.failed.append("%s %s: %s at %d of %d elements, first at flat index %d: got %.9g, want %.9g"
                               % (self.tag, name, what, int(bad.sum()), bad.numel(), i,
                                  float(got.reshape(-1)[i]), float(want.reshape(-1)[i])))

    def bounded(self, name, got, ref, mag, exact=False, slack=0.0):
        if got.shape != ref.shape:
            self.worst[name] = math.inf
            if not self.measure:
                self.failed.append("%s %s: shape %s, want %s" % (self.tag, name, tuple(got.shape), tuple(ref.shape)))
            return
        self.ratio(name, got, ref, mag, u_of(got.dtype), slack)
        if exact:
            self.same(name, got, ref.to(got.dtype), "not the exact value")


# ------------------------------------------------------------------ inputs
def _gen(*key):
    seed = 12345
    for i, k in enumerate(key):
        seed = (seed * 1000003 + int(k) * (7919 + 2 * i)) % (2 ** 31 - 1)
    return torch.Generator("cpu").manual_seed(seed)


def fam(family, shape, g, dtype=F32):
    shape = tuple(shape)
    if family == "gauss":
        t = torch.randn(shape, generator=g)
    elif family == "quarter":
        t = torch.relu(torch.randint(-8, 9, shape, generator=g).float() / 4)
    elif family == "negative":
        t = -(0.25 + torch.randn(shape, generator=g).abs())
    elif family == "signed_zero":
        t = torch.randn(shape, generator=g)
        r = torch.randint(0, 4, shape, generator=g)
        t = torch.where(r == 0, torch.tensor(0.0), t)
        t = torch.where(r == 1, torch.tensor(-0.0), t)
    elif family == "integers":
        t = torch.randint(-4, 5, shape, generator=g).float()
    else:
        raise KeyError(family)
    return t.to(dtype)


def _key(family, dtype, *dims):
    return (FAMILIES.index(family), 1 if dtype == BF else 0) + tuple(dims)


def relu_ref(x):
    """act of the kernels: x > 0 ? x : +0"""
    return torch.where(x > 0, x, torch.zeros((), dtype=x.dtype, device=x.device))


def out_hw(H, W, stride=2):
    return (H - 1) // stride + 1, (W - 1) // stride + 1


def _dev(c):
    return c.get("device", "cpu")


def _t(c, name, dt=F32):
    return c[name].to(device=_dev(c), dtype=dt)


def _cpu(o):
    return {k: (v.cpu() if torch.is_tensor(v) else v) for k, v in o.items()}


# ===================================================================== bilinear x2, align_corners=True
def bl_axis(n, dt=F64, mut=None):
    """source coordinate, the two taps and the second tap's weight of the 2n outputs along an axis of n inputs.
    F64: the reference (last output: taps (n - 2, n - 1), w1 = 1).  F32: as the kernels form them."""
    d = torch.arange(2 * n, dtype=dt)
    if mut == "bl_half_pixel":
        s = ((d + 0.5) / 2 - 0.5).clamp_min(0)
    elif dt == F64:
        s = d * (n - 1) / (2 * n - 1)
    else:
        scale = torch.tensor(float(n - 1), dtype=dt) / torch.tensor(float(2 * n - 1), dtype=dt) if n > 1 \
            else torch.tensor(0.0, dtype=dt)
        s = scale * d
    i0 = s.floor().long().clamp_max(max(n - 2, 0) if dt == F64 else n - 1)
    i1 = i0 + 1 if mut == "bl_no_clamp" else (i0 + 1).clamp_max(n - 1)
    return s, i0, i1, s - i0.to(dt)


def bl_matrix(n, dt=F64):
    """A [2n, n]: out = A in;  G: second tap minus first tap;  S: |error of the weight| / 2^-23 at the taps"""
    s, i0, i1, w1 = bl_axis(n, dt)
    o = torch.arange(2 * n)
    A, G, S = (torch.zeros(2 * n, n, dtype=dt) for _ in range(3))
    A.index_put_((o, i0), 1 - w1, accumulate=True)
    A.index_put_((o, i1), w1, accumulate=True)
    G.index_put_((o, i0), -torch.ones_like(w1), accumulate=True)
    G.index_put_((o, i1), torch.ones_like(w1), accumulate=True)
    S.index_put_((o, i0), s, accumulate=True)
    S.index_put_((o, i1), s, accumulate=True)
    S = torch.where(i0[:, None] == i1[:, None], torch.zeros_like(S), S)     # n = 1: one tap of weight 1
    return A, G, S, s


def bilinear_case(family, B, H, W, C, dtype, seed=0):
    g = _gen(1, seed, *_key(family, dtype, B, H, W, C))
    return {"kind": "bilinear", "family": family, "dtype": dtype, "shape": (B, H, W, C),
            "x": fam(family, (B, H, W, C), g, dtype), "dy": fam(family, (B, 2 * H, 2 * W, C), g, dtype)}


def bilinear_ref(c):
    B, H, W, C = c["shape"]
    x = c["x"].to(F64).requires_grad_(True)
    dy = c["dy"].to(F64)
    y = Fn.interpolate(x.permute(0, 3, 1, 2), scale_factor=2, mode="bilinear", align_corners=True).permute(0, 2, 3, 1)
    dx, = torch.autograd.grad(y, x, dy)
    x = x.detach()
    Ay, Gy, Sy, sy = bl_matrix(H)
    Ax, Gx, Sx, sx = bl_matrix(W)
    e = torch.einsum
    r = {"y": y.detach(), "dx": dx,
         "t_y": e("oh,bhwc,pw->bopc", Ay, x.abs(), Ax), "t_dx": e("oh,bopc,pw->bhwc", Ay, dy.abs(), Ax)}
    Dx = e("oh,bhpc->bopc", Ay, e("bhwc,pw->bhpc", x, Gx).abs()) * sx.view(1, 1, -1, 1)
    Dy = e("bowc,pw->bopc", e("oh,bhwc->bowc", Gy, x).abs(), Ax) * sy.view(1, -1, 1, 1)
    r["s_y"] = 2 * EPS32 * (Dx + Dy)
    r["s_dx"] = 2 * EPS32 * (e("oh,bopc,pw->bhwc", Ay, dy.abs(), Sx) + e("oh,bopc,pw->bhwc", Sy, dy.abs(), Ax))
    return r


def bilinear_eval(c, mut=None, dt=F32):
    B, H, W, C = c["shape"]
    dev = _dev(c)
    x, dy = _t(c, "x", dt), _t(c, "dy", dt)
    _, y0, y1, wy = (t.to(dev) for t in bl_axis(H, dt, mut))
    _, x0, x1, wx = (t.to(dev) for t in bl_axis(W, dt, mut))
    # what lies behind the map is not the map's: the unclamped second tap (weight 0) reads it
    flat = torch.cat([x.reshape(-1, C), torch.full((W + 2, C), float("nan"), dtype=dt, device=dev)])
    b = torch.arange(B, device=dev).view(B, 1, 1)
    tap = lambda yy, xx: flat[(b * H + yy.view(1, -1, 1)) * W + xx.view(1, 1, -1)]
    wyv, wxv = wy.view(1, -1, 1, 1), wx.view(1, 1, -1, 1)
    if mut == "bl_xy_swapped":
        top = (1 - wyv) * tap(y0, x0) + wyv * tap(y0, x1)
        bot = (1 - wyv) * tap(y1, x0) + wyv * tap(y1, x1)
        y = (1 - wxv) * top + wxv * bot
    else:
        top = (1 - wxv) * tap(y0, x0) + wxv * tap(y0, x1)
        bot = (1 - wxv) * tap(y1, x0) + wxv * tap(y1, x1)
        y = (1 - wyv) * top + wyv * bot

    def mat(n):
        _, i0, i1, w1 = (t.to(dev) for t in bl_axis(n, dt))
        o = torch.arange(2 * n, device=dev)
        A = torch.zeros(2 * n, n, dtype=dt, device=dev)
        A.index_put_((o, i0), 1 - w1, accumulate=True)
        A.index_put_((o, i1), w1, accumulate=True)
        if mut == "bl_bwd_last_candidate_dropped":      # the candidate window cut one output short
            A = torch.where(o[:, None] == 2 * torch.arange(n, device=dev)[None, :] + 2, torch.zeros_like(A), A)
        return A
    dx = torch.einsum("oh,bopc,pw->bhwc", mat(H), dy, mat(W))
    return _cpu({"y": y.to(c["dtype"]), "dx": dx.to(c["dtype"])})


def bilinear_check(c, o, rep):
    r = bilinear_ref(c)
    rep.bounded("bl_fwd", o["y"], r["y"], r["t_y"], slack=r["s_y"])
    rep.bounded("bl_bwd", o["dx"], r["dx"], r["t_dx"], slack=r["s_dx"])


# ===================================================================== MaxPool2d(3, 2, 1)
def pool3_case(family, B, H, W, C, dtype, seed=0):
    g = _gen(2, seed, *_key(family, dtype, B, H, W, C))
    Ho, Wo = out_hw(H, W)
    return {"kind": "pool3", "family": family, "dtype": dtype, "shape": (B, H, W, C),
            "x": fam(family, (B, H, W, C), g, dtype),
            "dy": fam("integers" if family == "integers" else "gauss", (B, Ho, Wo, C), g, dtype)}


def pool3_ref(x):
    """values (x's dtype) and arg bytes (dy * 3 + dx of the first maximum; ATen: a NaN anywhere wins)"""
    B, H, W, C = x.shape
    v, idx = Fn.max_pool2d(x.to(F64).permute(0, 3, 1, 2), 3, 2, 1, return_indices=True)
    Ho, Wo = v.shape[2:]
    oy, ox = torch.arange(Ho).view(Ho, 1), torch.arange(Wo).view(1, Wo)
    arg = (idx // W - (2 * oy - 1)) * 3 + (idx % W - (2 * ox - 1))
    return v.permute(0, 2, 3, 1).contiguous().to(x.dtype), arg.permute(0, 2, 3, 1).contiguous().to(torch.uint8)


def pool3_bwd(dy, arg, H, W, dt=F64, swapped=False):
    """dx and the sum of |dy| routed to each pixel, from the arg bytes as given"""
    B, Ho, Wo, C = dy.shape
    a = arg.long()
    dyy, dxx = (a % 3, a // 3) if swapped else (a // 3, a % 3)
    iy = 2 * torch.arange(Ho, device=dy.device).view(1, Ho, 1, 1) - 1 + dyy
    ix = 2 * torch.arange(Wo, device=dy.device).view(1, 1, Wo, 1) - 1 + dxx
    ok = (a < 9) & (iy >= 0) & (iy < H) & (ix >= 0) & (ix < W)
    flat = ((torch.arange(B, device=dy.device).view(B, 1, 1, 1) * H + iy) * W + ix) * C \
        + torch.arange(C, device=dy.device).view(1, 1, 1, C)
    g = dy.to(dt)
    dx = torch.zeros(B * H * W * C, dtype=dt, device=dy.device).index_add_(0, flat[ok], g[ok])
    mag = torch.zeros(B * H * W * C, dtype=dt, device=dy.device).index_add_(0, flat[ok], g[ok].abs())
    return dx.view(B, H, W, C), mag.view(B, H, W, C)


def _first(eq, last=False):
    """index along dim -2 of the first (last) True"""
    n = eq.shape[-2]
    pos = torch.arange(n, device=eq.device).view(n, 1)
    return (eq * ((pos + 1) if last else (n - pos))).argmax(-2)


def pool3_eval(c, mut=None, dt=F32):
    B, H, W, C = c["shape"]
    x, dy = _t(c, "x", dt), _t(c, "dy", dt)
    Ho, Wo = out_hw(H, W)
    xp = Fn.pad(x.permute(0, 3, 1, 2), (1, 1, 1, 1), value=0.0 if mut == "pool_pad_zero" else -math.inf)
    win = Fn.unfold(xp, 3, stride=2).view(B, C, 9, Ho, Wo).permute(0, 3, 4, 2, 1)       # [B, Ho, Wo, 9, C]
    m = win.max(-2).values
    arg = _first(win == m.unsqueeze(-2), last=mut == "pool_last_max").to(torch.uint8)
    dx = pool3_bwd(dy, arg, H, W, dt, swapped=mut == "pool_bwd_arg_swapped")[0]
    if mut == "pool_floor_output" and (H % 2 or W % 2):
        m, arg = m[:, :max(H // 2, 1), :max(W // 2, 1)], arg[:, :max(H // 2, 1), :max(W // 2, 1)]
    return _cpu({"y": m.to(c["dtype"]).contiguous(), "arg": arg.contiguous(), "dx": dx.to(c["dtype"])})


def pool3_check(c, o, rep):
    B, H, W, C = c["shape"]
    y, arg = pool3_ref(c["x"])
    rep.same("pool_y", o["y"], y, "not the window's maximum")
    rep.same("pool_arg", o["arg"], arg, "not the first maximum's position")
    if o["arg"].shape == c["dy"].shape:
        dx, mag = pool3_bwd(c["dy"], o["arg"], H, W)
        rep.bounded("pool_dx", o["dx"], dx, mag, exact=c["family"] == "integers")


# ===================================================================== MaxPool2d(2)
def pool2_case(family, B, H, W, C, dtype, seed=0):
    g = _gen(3, seed, *_key(family, dtype, B, H, W, C))
    return {"kind": "pool2", "family": family, "dtype": dtype, "shape": (B, H, W, C),
            "x": fam(family, (B, H, W, C), g, dtype), "dy": fam("gauss", (B, H // 2, W // 2, C), g, dtype)}


def pool2_ref(x, dy):
    v, idx = Fn.max_pool2d(x.to(F64).permute(0, 3, 1, 2), 2, return_indices=True)
    B, C, Ho, Wo = v.shape
    g = dy.permute(0, 3, 1, 2).reshape(B, C, -1)
    dx = torch.zeros(B, C, x.shape[1] * x.shape[2], dtype=dy.dtype).scatter_(2, idx.view(B, C, -1), g)
    return v.permute(0, 2, 3, 1).contiguous().to(x.dtype), dx.view(B, C, x.shape[1], x.shape[2]).permute(0, 2, 3, 1).contiguous()


def pool2_eval(c, mut=None, dt=F32):
    B, H, W, C = c["shape"]
    x, dy = _t(c, "x", dt), _t(c, "dy", dt)
    win = x.view(B, H // 2, 2, W // 2, 2, C).permute(0, 1, 3, 2, 4, 5).reshape(B, H // 2, W // 2, 4, C)
    m = win.max(-2).values
    t = _first(win == m.unsqueeze(-2), last=mut == "pool2_last_max")
    dwin = torch.where(torch.arange(4, device=x.device).view(4, 1) == t.unsqueeze(-2), dy.unsqueeze(-2),
                       torch.zeros((), dtype=dt, device=x.device))
    dx = dwin.view(B, H // 2, W // 2, 2, 2, C).permute(0, 1, 3, 2, 4, 5).reshape(B, H, W, C)
    return _cpu({"y": m.to(c["dtype"]), "dx": dx.to(c["dtype"])})


def pool2_check(c, o, rep):
    y, dx = pool2_ref(c["x"], c["dy"])
    rep.same("pool2_y", o["y"], y, "not the window's maximum")
    rep.same("pool2_dx", o["dx"], dx, "not dy at the first maximum, 0 elsewhere")


# ===================================================================== global average pool
def avg_case(family, B, HW, C, dtype, seed=0):
    g = _gen(4, seed, *_key(family, dtype, B, HW, C))
    return {"kind": "avg", "family": family, "dtype": dtype, "shape": (B, HW, C),
            "x": fam(family, (B, HW, 1, C), g, dtype), "dy": fam("gauss", (B, C), g)}


def avg_eval(c, mut=None, dt=F32):
    B, HW, C = c["shape"]
    x, dy = _t(c, "x", dt).reshape(-1, C), _t(c, "dy", dt)
    stride = HW - 1 if mut == "avg_batch_stride" else HW
    s = torch.zeros(B, C, dtype=dt, device=x.device)
    first = torch.arange(B, device=x.device) * stride
    for r in range(HW):             # the kernel's running sum
        s = s + x[first + r]
    y = s / torch.tensor(float(HW + 1 if mut == "avg_divisor" else HW), dtype=dt)
    dx = (dy / torch.tensor(float(HW), dtype=dt)).view(B, 1, 1, C).expand(B, HW, 1, C)
    return _cpu({"y": y, "dx": dx.to(c["dtype"]).contiguous()})


def avg_check(c, o, rep):
    B, HW, C = c["shape"]
    x = c["x"].to(F64).view(B, HW, C)
    rep.bounded("avg_fwd", o["y"], x.mean(1), x.abs().mean(1), exact=c["family"] == "integers" and HW & (HW - 1) == 0)
    ref = (c["dy"].to(F64) / HW).view(B, 1, 1, C).expand(B, HW, 1, C)
    rep.bounded("avg_bwd", o["dx"], ref, ref.abs())


# ===================================================================== 3x3 patch matrix and its transpose
def im2col_case(family, B, H, W, C, stride, ld, relu, dtype, seed=0):
    g = _gen(5, seed, *_key(family, dtype, B, H, W, C, stride, ld, relu))
    Ho, Wo = out_hw(H, W, stride)
    return {"kind": "im2col", "family": family, "dtype": dtype, "shape": (B, H, W, C), "stride": stride, "ld": ld,
            "relu": relu, "x": fam(family, (B, H, W, C), g, dtype),
            "dcols": fam("integers" if family == "integers" else "gauss", (B * Ho * Wo, ld), g, dtype)}


def im2col_ref(x, stride, ld, relu):
    B, H, W, C = x.shape
    a = relu_ref(x) if relu else x
    u = Fn.unfold(a.float().permute(0, 3, 1, 2), 3, padding=1, stride=stride)        # [B, (c, dy, dx), L]
    L = u.shape[2]
    cols = u.view(B, C, 9, L).permute(0, 3, 2, 1).reshape(B * L, 9 * C)
    return Fn.pad(cols, (0, ld - 9 * C)).to(x.dtype)


def col2im_ref(dcols, B, H, W, C, stride):
    """-> dx, sum of |terms| (fp64)"""
    L = dcols.shape[0] // B
    u = dcols[:, :9 * C].to(F64).view(B, L, 9, C).permute(0, 3, 2, 1).reshape(B, C * 9, L)
    f = lambda t: Fn.fold(t, (H, W), 3, padding=1, stride=stride).permute(0, 2, 3, 1)
    return f(u), f(u.abs())


def im2col_eval(c, mut=None, dt=F32):
    B, H, W, C = c["shape"]
    s, ld, dev = c["stride"], c["ld"], _dev(c)
    x, dcols = _t(c, "x", dt), _t(c, "dcols", dt)
    Ho, Wo = out_hw(H, W, s)
    a = relu_ref(x) if c["relu"] and mut != "im2col_no_relu" else x
    off = 1 if mut == "im2col_centre_off" and s == 2 else 0
    xp = Fn.pad(a, (0, 0, 1, 2 + off, 1, 2 + off))
    taps = []
    for t in range(9):
        dy, dx = (t % 3, t // 3) if mut == "im2col_tap_order" else (t // 3, t % 3)
        taps.append(xp[:, dy + off:dy + off + s * Ho:s, dx + off:dx + off + s * Wo:s])
    cols = torch.stack(taps, 3).reshape(B * Ho * Wo, 9 * C)
    cols = Fn.pad(cols, (0, ld - 9 * C), value=1.0 if mut == "im2col_pad_not_zero" else 0.0)
    # the transpose in the kernel's gather form
    d5 = dcols[:, :9 * C].view(B, Ho, Wo, 9, C)
    acc = torch.zeros(B, H, W, C, dtype=dt, device=dev)
    for t in range(9):
        ny, nx = torch.arange(H, device=dev) + 1 - t // 3, torch.arange(W, device=dev) + 1 - t % 3
        par = (lambda n: torch.ones_like(n, dtype=torch.bool)) if mut == "col2im_no_parity" else (lambda n: n % s == 0)
        vy, vx = (ny >= 0) & par(ny) & (ny // s < Ho), (nx >= 0) & par(nx) & (nx // s < Wo)
        oy, ox = (ny // s).clamp(0, Ho - 1), (nx // s).clamp(0, Wo - 1)
        term = d5[:, oy][:, :, ox][:, :, :, t]
        acc = acc + torch.where((vy.view(-1, 1) & vx.view(1, -1)).view(1, H, W, 1), term, torch.zeros_like(term))
    return _cpu({"cols": cols.to(c["dtype"]), "dx": acc.to(c["dtype"])})


def im2col_check(c, o, rep):
    B, H, W, C = c["shape"]
    rep.same("im2col", o["cols"], im2col_ref(c["x"], c["stride"], c["ld"], c["relu"]), "not the (dy, dx, c) patch matrix")
    dx, mag = col2im_ref(c["dcols"], B, H, W, C, c["stride"])
    rep.bounded("col2im", o["dx"], dx, mag, exact=c["family"] == "integers")


# ===================================================================== stem patch matrix
def stem_case(B, H, W, dtype, seed=0):
    g = _gen(6, seed, *_key("gauss", dtype, B, H, W))
    return {"kind": "stem", "family": "gauss", "dtype": dtype, "shape": (B, H, W), "ld": 192 if dtype == BF else 152,
            "img": torch.randn(B, 3, H, W, generator=g)}


def stem_eval(c, mut=None, dt=F32):
    B, H, W = c["shape"]
    img = _t(c, "img", dt)
    Ho, Wo = out_hw(H, W)
    p = 2 if mut == "stem_pad_2" else 3
    xp = Fn.pad(img, (p, p + 4, p, p + 4))
    taps = [xp[:, :, t // 7:t // 7 + 2 * Ho:2, t % 7:t % 7 + 2 * Wo:2] for t in range(49)]      # each [B, 3, Ho, Wo]
    st = torch.stack(taps, 0)                                                                      # [49, B, 3, Ho, Wo]
    cols = (st.permute(1, 3, 4, 2, 0) if mut == "stem_channel_outermost" else st.permute(1, 3, 4, 0, 2)) \
        .reshape(B * Ho * Wo, 147)
    return _cpu({"cols": Fn.pad(cols, (0, c["ld"] - 147)).to(c["dtype"])})


def stem_check(c, o, rep):
    B, H, W = c["shape"]
    u = Fn.unfold(c["img"], 7, padding=3, stride=2)
    L = u.shape[2]
    cols = u.view(B, 3, 49, L).permute(0, 3, 2, 1).reshape(B * L, 147)
    rep.same("stem", o["cols"], Fn.pad(cols, (0, c["ld"] - 147)).to(c["dtype"]), "not the (dy, dx, c) stem patch matrix")


# ===================================================================== stride-2 subsampling
def sub_case(family, B, H, W, C, dtype, seed=0):
    g = _gen(7, seed, *_key(family, dtype, B, H, W, C))
    Ho, Wo = out_hw(H, W)
    return {"kind": "sub", "family": family, "dtype": dtype, "shape": (B, H, W, C),
            "x": fam(family, (B, H, W, C), g, dtype), "dy": fam(family, (B, Ho, Wo, C), g, dtype)}


def sub_eval(c, mut=None, dt=F32):
    B, H, W, C = c["shape"]
    x, dy = _t(c, "x", dt), _t(c, "dy", dt)
    if mut == "sub_bwd_odd_filled":
        dx = dy.repeat_interleave(2, 1).repeat_interleave(2, 2)[:, :H, :W]
    else:
        dx = torch.zeros_like(x)
        dx[:, ::2, ::2] = dy
    return _cpu({"y": x[:, ::2, ::2].contiguous().to(c["dtype"]), "dx": dx.contiguous().to(c["dtype"])})


def sub_check(c, o, rep):
    dx = torch.zeros_like(c["x"])
    dx[:, ::2, ::2] = c["dy"]
    rep.same("sub_fwd", o["y"], c["x"][:, ::2, ::2].contiguous(), "not x[:, ::2, ::2]")
    rep.same("sub_bwd", o["dx"], dx, "not dy at the even positions, +0 elsewhere")


# ===================================================================== ConvTranspose2d(k = s) scatter
def shuffle_case(family, B, H, W, k, C, dtype, seed=0):
    g = _gen(8, seed, *_key(family, dtype, B, H, W, k, C))
    return {"kind": "shuffle", "family": family, "dtype": dtype, "shape": (B, H, W, C), "k": k,
            "g": fam(family, (B * H * W, k * k * C), g, dtype), "bias": fam(family, (C,), g)}


def shuffle_index(g, B, H, W, k, C, swapped=False):
    v = g.view(B, H, W, k, k, C)
    return (v.permute(0, 1, 4, 2, 3, 5) if swapped else v.permute(0, 1, 3, 2, 4, 5)).reshape(B, k * H, k * W, C)


def shuffle_eval(c, mut=None, dt=F32):
    B, H, W, C = c["shape"]
    k = c["k"]
    g, bias = _t(c, "g", dt), _t(c, "bias", dt)
    y = shuffle_index(g, B, H, W, k, C, swapped=mut == "shuffle_ij_swapped")
    if mut == "shuffle_bias_by_chunk":
        bias = bias[torch.arange(C, device=g.device) // V(c["dtype"])]
    back = y.view(B, H, k, W, k, C).permute(0, 1, 3, 2, 4, 5).reshape(B * H * W, k * k * C)
    return _cpu({"y": y.contiguous().to(c["dtype"]), "yb": (y + bias).to(c["dtype"]), "dg": back.to(c["dtype"])})


def shuffle_check(c, o, rep):
    B, H, W, C = c["shape"]
    y = shuffle_index(c["g"], B, H, W, c["k"], C).contiguous()
    rep.same("shuffle", o["y"], y, "not g at (i, j, c) of its pixel")
    rep.same("unshuffle", o["dg"], c["g"], "unshuffle(shuffle(g)) is not g")
    b = c["bias"].to(F64)
    rep.bounded("shuffle_bias", o["yb"], y.to(F64) + b, y.to(F64).abs() + b.abs(), exact=c["family"] == "integers")


# ===================================================================== tokens <-> map
def tokens_case(family, B, L, D, dtype, seed=0):
    g = _gen(9, seed, *_key(family, dtype, B, L, D))
    return {"kind": "tokens", "family": family, "dtype": dtype, "shape": (B, L, D),
            "z": fam(family, (B, L + 1, D), g), "dx": fam(family, (B * L, D), g, dtype)}


def tokens_eval(c, mut=None, dt=F32):
    B, L, D = c["shape"]
    z, dx = _t(c, "z", dt), _t(c, "dx", dt)
    x = (z[:, :L] if mut == "tokens_cls_kept" else z[:, 1:]).reshape(B * L, D)
    first = dx.view(B, L, D)[:, :1] if mut == "tokens_cls_not_zeroed" else torch.zeros(B, 1, D, dtype=dt, device=z.device)
    return _cpu({"x": x.to(c["dtype"]), "dz": torch.cat([first, dx.view(B, L, D)], 1).float()})


def tokens_check(c, o, rep):
    B, L, D = c["shape"]
    rep.same("tok2map", o["x"], c["z"][:, 1:].reshape(B * L, D).to(c["dtype"]), "not the token rows in the operand type")
    want = torch.cat([torch.zeros(B, 1, D), c["dx"].view(B, L, D).float()], 1)
    rep.same("map2tok", o["dz"], want, "not [+0 | dx]")


# ===================================================================== pointwise: add, ReLU backward (+ skip), GELU
def eltwise_case(family, n, dtype, seed=0):
    g = _gen(10, seed, family == "grid", *_key("gauss" if family == "grid" else family, dtype, n))
    grid = torch.linspace(-8, 8, n) if family == "grid" else None      # gelu_map over [-8, 8]
    return {"kind": "eltwise", "family": family, "dtype": dtype, "shape": (n,),
            "a": (grid if grid is not None else fam(family, (n,), g)).to(dtype),
            "b": fam("gauss" if family == "grid" else family, (n,), g, dtype),
            "s": fam("gauss" if family == "grid" else family, (n,), g, dtype)}


def gelu_tanh(x):
    return 0.5 * x * (1 + torch.tanh(0.7978845608028654 * (x + 0.044715 * x ** 3)))


def eltwise_eval(c, mut=None, dt=F32):
    a, b, s = _t(c, "a", dt), _t(c, "b", dt), _t(c, "s", dt)
    lp = c["dtype"]
    masked = torch.where((b if mut == "relu_bwd_mask_from_g" else a) > 0, b, torch.zeros_like(b)).to(lp)
    cdf = 0.5 * (1 + torch.erf(a * 0.7071067811865476))
    gl = gelu_tanh(a) if mut == "gelu_tanh_form" and lp == F32 else 0.5 * a * (1 + torch.erf(a * 0.7071067811865476))
    dgl = b * (cdf + a * (0.3989422804014327 * torch.exp(-0.5 * a * a)))
    return _cpu({"add": (a + b).to(lp), "relu_bwd": masked, "relu_bwd_skip": (masked.to(dt) + s).to(lp),
                 "gelu": gl.to(lp), "dgelu": dgl.to(lp)})


def eltwise_check(c, o, rep):
    a, b, s = c["a"], c["b"], c["s"]
    masked = torch.where(a > 0, b, torch.zeros_like(b))
    rep.same("add", o["add"], a + b, "not a + b in the tensor's dtype")
    rep.same("relu_bwd", o["relu_bwd"], masked, "not x > 0 ? g : +0")
    rep.same("relu_bwd", o["relu_bwd_skip"], masked + s, "not (x > 0 ? g : 0) + skip in the tensor's dtype")
    x = a.to(F64).requires_grad_(True)
    y = Fn.gelu(x)
    d, = torch.autograd.grad(y, x, b.to(F64))
    xd = x.detach()
    rep.bounded("gelu_fwd", o["gelu"], y.detach(), xd.abs())
    phi = torch.exp(-0.5 * xd * xd) / math.sqrt(2 * math.pi)
    rep.bounded("gelu_bwd", o["dgelu"], d, b.to(F64).abs() * (1 + xd.abs() * phi))


# ===================================================================== depth head
def head_case(family, M, C, dtype, accumulate=False, seed=0):
    g = _gen(11, seed, *_key(family, dtype, M, C, accumulate))
    return {"kind": "head", "family": family, "dtype": dtype, "shape": (M, C), "x": fam(family, (M, C), g, dtype),
            "w": 0.5 * torch.randn(C, generator=g), "bias": 0.3 * torch.randn(1, generator=g),
            "dy": fam("integers" if family == "integers" else "gauss", (M,), g),
            "dw0": torch.randn(C, generator=g) if accumulate else None,
            "db0": torch.randn(1, generator=g) if accumulate else None}


def head_eval(c, mut=None, dt=F32):
    M, C = c["shape"]
    x, w, bias, dy = _t(c, "x", dt), _t(c, "w", dt), _t(c, "bias", dt), _t(c, "dy", dt)
    r = relu_ref(x)
    y = 1 / (1 + torch.exp(-(bias + (r * w).sum(1))))
    ds = dy * y * ((1 + y) if mut == "head_derivative" else (1 - y))
    on = (x >= 0) if mut == "head_mask_ge" else (x > 0)
    dx = torch.where(on, ds[:, None] * w, torch.zeros((), dtype=dt, device=x.device))
    n = HEAD_GRID_ROWS if mut == "head_first_sweep_only" else M
    dw, db = (ds[:n, None] * r[:n]).sum(0), ds[:n].sum().view(1)
    if c["dw0"] is not None:
        dw, db = dw + _t(c, "dw0", dt), db + _t(c, "db0", dt)
    return _cpu({"y": y.float(), "dx": dx.to(c["dtype"]), "dw": dw.float(), "db": db.float()})


def head_check(c, o, rep):
    x, w, bias = c["x"].to(F64), c["w"].to(F64), c["bias"].to(F64)
    r = relu_ref(x)
    s, t = bias + (r * w).sum(1), bias.abs() + (r * w).abs().sum(1)
    y = torch.sigmoid(s)
    rep.bounded("head_y", o["y"], y, y * (1 - y) * t + y)
    yk = o["y"].to(F64)                 # the backward starts from the y it is handed
    ds = c["dy"].to(F64) * yk * (1 - yk)
    dx = torch.where(x > 0, ds[:, None] * w, torch.zeros((), dtype=F64))
    rep.bounded("head_dx", o["dx"], dx, (ds[:, None] * w).abs().expand_as(dx))
    dw, tw, db, tb = (ds[:, None] * r).sum(0), (ds[:, None] * r).abs().sum(0), ds.sum().view(1), ds.abs().sum().view(1)
    if c["dw0"] is not None:
        dw, tw = dw + c["dw0"].to(F64), tw + c["dw0"].to(F64).abs()
        db, tb = db + c["db0"].to(F64), tb + c["db0"].to(F64).abs()
    rep.bounded("head_dw", o["dw"], dw, tw)
    rep.bounded("head_db", o["db"], db, tb)


# ===================================================================== momentum update
def ema_case(family, n, m, seed=0):
    g = _gen(12, seed, *_key(family, F32, n, int(m * 1000)))
    return {"kind": "ema", "family": family, "dtype": F32, "shape": (n,), "m": m,
            "dst": fam(family, (n,), g), "src": fam(family, (n,), g)}


def ema_eval(c, mut=None, dt=F32):
    dst, src = _t(c, "dst", dt), _t(c, "src", dt)
    m = torch.tensor(c["m"], dtype=dt)
    a, b = (1 - m, m) if mut == "ema_swapped" else (m, 1 - m)
    out = dst * a + src * b
    n = dst.numel()
    if mut == "ema_tail_skipped" and n % 4:
        out[n - n % 4:] = dst[n - n % 4:]
    return _cpu({"out": out.float()})


def ema_check(c, o, rep):
    m = float(torch.tensor(c["m"], dtype=F32))
    d, s = c["dst"].to(F64) * m, c["src"].to(F64) * (1 - m)
    rep.bounded("ema", o["out"], d + s, d.abs() + s.abs(), exact=c["family"] == "integers" and c["m"] in (0, 1))


# ===================================================================== table
# kind -> (case constructor, fp32 evaluation, check)
KINDS = {"bilinear": (bilinear_case, bilinear_eval, bilinear_check), "pool3": (pool3_case, pool3_eval, pool3_check),
         "pool2": (pool2_case, pool2_eval, pool2_check), "avg": (avg_case, avg_eval, avg_check),
         "im2col": (im2col_case, im2col_eval, im2col_check), "stem": (stem_case, stem_eval, stem_check),
         "sub": (sub_case, sub_eval, sub_check), "shuffle": (shuffle_case, shuffle_eval, shuffle_check),
         "tokens": (tokens_case, tokens_eval, tokens_check), "eltwise": (eltwise_case, eltwise_eval, eltwise_check),
         "head": (head_case, head_eval, head_check), "ema": (ema_case, ema_eval, ema_check)}
# deliberately wrong fp32 evaluations: name -> (kind, the check that must catch it)
MUTATIONS = {
    "bl_half_pixel": ("bilinear", "bl_fwd"),                    # align_corners=False coordinates
    "bl_xy_swapped": ("bilinear", "bl_fwd"),                    # x and y weights exchanged
    "bl_no_clamp": ("bilinear", "bl_fwd"),                      # i1 = i0 + 1: weight 0 times what lies behind the map
    "bl_bwd_last_candidate_dropped": ("bilinear", "bl_bwd"),    # the last contributing output row and column
    "pool_last_max": ("pool3", "pool_arg"),
    "pool_pad_zero": ("pool3", "pool_y"),
    "pool_floor_output": ("pool3", "pool_y"),                   # Ho = H / 2 for odd H
    "pool_bwd_arg_swapped": ("pool3", "pool_dx"),               # the arg read as dx * 3 + dy
    "pool2_last_max": ("pool2", "pool2_dx"),
    "avg_divisor": ("avg", "avg_fwd"),                          # HW + 1
    "avg_batch_stride": ("avg", "avg_fwd"),                     # images HW - 1 rows apart
    "im2col_tap_order": ("im2col", "im2col"),                   # (dx, dy)
    "im2col_pad_not_zero": ("im2col", "im2col"),
    "im2col_centre_off": ("im2col", "im2col"),                  # stride 2 centred at 2 o + 1
    "im2col_no_relu": ("im2col", "im2col"),
    "col2im_no_parity": ("im2col", "col2im"),
    "shuffle_ij_swapped": ("shuffle", "shuffle"),
    "shuffle_bias_by_chunk": ("shuffle", "shuffle_bias"),
    "tokens_cls_kept": ("tokens", "tok2map"),
    "tokens_cls_not_zeroed": ("tokens", "map2tok"),
    "head_mask_ge": ("head", "head_dx"),
    "head_derivative": ("head", "head_dx"),                     # y (1 + y)
    "head_first_sweep_only": ("head", "head_dw"),               # dw / db over the first 262144 rows
    "gelu_tanh_form": ("eltwise", "gelu_fwd"),
    "ema_swapped": ("ema", "ema"),
    "ema_tail_skipped": ("ema", "ema"),
    "relu_bwd_mask_from_g": ("eltwise", "relu_bwd"),
    "stem_pad_2": ("stem", "stem"),
    "stem_channel_outermost": ("stem", "stem"),
    "sub_bwd_odd_filled": ("sub", "sub_bwd"),
}


def make(kind, args):
    return KINDS[kind][0](*args)


def to_device(c, device):
    """the case with `device` noted: the fp32 evaluation moves what it needs, the references stay on the CPU"""
    return dict(c, device=device)


def run_check(c, o, tag="", measure=False, k=None):
    rep = Report(tag or "%s %s %s %s" % (c["kind"], c["family"], dname(c["dtype"]), c["shape"]), measure, k)
    KINDS[c["kind"]][2](c, o, rep)
    return rep


def evaluate(c, mut=None):
    return KINDS[c["kind"]][1](c, mut if mut is not None and MUTATIONS[mut][0] == c["kind"] else None)


# ------------------------------------------------------------------ the case list of the GPU module
BL_SHAPES = lambda v: ((1, 1, 1, v), (2, 1, 5, v), (2, 5, 1, v), (1, 2, 2, v), (2, 3, 5, 2 * v), (1, 14, 14, 256),
                       (1, 9, 33, 128))
POOL3_MAPS = ((1, 1, 1), (1, 1, 5), (2, 5, 1), (1, 2, 2), (2, 7, 9), (2, 12, 10), (3, 14, 14))
POOL3_C = lambda dt: (V(dt), 3 * V(dt), 64) + ((3, 6) if dt == F32 else (4, 12))
POOL2_SHAPES = lambda v: ((1, 2, 2, v), (2, 12, 10, 16), (1, 14, 14, 256))
AVG_HW, AVG_C = (1, 49, 196), (3, 8, 256, 260, 2048)
IM2COL_MAPS = ((1, 1), (1, 6), (6, 1), (7, 9), (8, 8), (8, 9), (9, 8))
STEM_SHAPES = ((1, 1, 1), (2, 7, 9), (1, 8, 6), (2, 32, 31))
SUB_SHAPES = lambda v: ((1, 1, 1, v), (2, 7, 9, 2 * v), (2, 8, 6, v), (1, 14, 14, 64))
SHUFFLE_SHAPES = lambda v: ((1, 1, 1, v), (2, 5, 6, 24))
TOKEN_SHAPES = ((1, 1, 4), (2, 5, 12), (3, 196, 768))
ELTWISE_N = lambda v: (v, 255 * v, 256 * v, 257 * v, 4099 * v)
HEAD_C = lambda v: (v, 32, 64)
HEAD_M = (1, 240, 257)
HEAD_LONG = (HEAD_GRID_ROWS + 300, 8)
EMA_N, EMA_M = (1, 3, 4, 1023, 1024, 1025, 70001), (0, 0.99, 1)
DTYPES = (F32, BF)


def k_pad(k, dtype):
    """ssl4gie_amd.conv_plan.k_pad: whole 64-deep K-tiles for the bf16 MFMA GEMM"""
    return (k + 63) // 64 * 64 if dtype == BF else k


def gpu_specs(kind):
    """(group, arguments of the kind's case constructor) of every case tests/test_gpu_map_kernels.py runs"""
    out = []
    for dt in DTYPES:
        v, n = V(dt), dname(dt)
        if kind == "bilinear":
            for s in BL_SHAPES(v):
                for f in ("gauss", "integers") + (("negative",) if s[1] * s[2] <= 15 else ()):
                    out.append(("%s-%dx%dx%dx%d" % ((n,) + s), (f,) + s + (dt,)))
        elif kind == "pool3":
            for m in POOL3_MAPS:
                for C in POOL3_C(dt):
                    for f in ("gauss", "quarter", "negative", "integers"):
                        out.append(("%s-%dx%dx%d" % ((n,) + m), (f,) + m + (C, dt)))
        elif kind == "pool2":
            for s in POOL2_SHAPES(v):
                for f in ("gauss", "quarter", "negative"):
                    out.append(("%s-%dx%dx%dx%d" % ((n,) + s), (f,) + s + (dt,)))
        elif kind == "avg":
            for HW in AVG_HW:
                for C in AVG_C:
                    for f in ("gauss", "negative", "integers"):
                        out.append(("%s-hw%d" % (n, HW), (f, 3, HW, C, dt)))
        elif kind == "im2col":
            for stride in (1, 2):
                for i, (H, W) in enumerate(IM2COL_MAPS):
                    for C in (v, 3 * v):
                        for j, ld in enumerate((9 * C, 9 * C + 24, k_pad(9 * C, dt))):
                            if j == 2 and ld == 9 * C:
                                continue
                            f = ("signed_zero", "gauss", "integers")[(i + j) % 3]
                            out.append(("%s-s%d-%dx%d" % (n, stride, H, W),
                                        (f, 1 + i % 2, H, W, C, stride, ld, int(f != "gauss"), dt)))
        elif kind == "stem":
            for s in STEM_SHAPES:
                out.append(("%s-%dx%dx%d" % ((n,) + s), s + (dt,)))
        elif kind == "sub":
            for s in SUB_SHAPES(v):
                out.append(("%s-%dx%dx%dx%d" % ((n,) + s), ("signed_zero",) + s + (dt,)))
        elif kind == "shuffle":
            for k in (2, 4):
                for (B, H, W, C) in SHUFFLE_SHAPES(v):
                    for f in ("gauss", "integers"):
                        out.append(("%s-k%d-%dx%dx%dx%d" % (n, k, B, H, W, C), (f, B, H, W, k, C, dt)))
        elif kind == "tokens":
            for s in TOKEN_SHAPES:
                out.append(("%s-%dx%dx%d" % ((n,) + s), ("signed_zero",) + s + (dt,)))
        elif kind == "eltwise":
            for nn in ELTWISE_N(v):
                for f in ("gauss", "signed_zero", "grid"):
                    out.append(("%s-n%d" % (n, nn), (f, nn, dt)))
        elif kind == "head":
            for C in HEAD_C(v):
                for i, M in enumerate(HEAD_M):
                    for j, f in enumerate(("gauss", "signed_zero", "quarter")):
                        out.append(("%s-c%d" % (n, C), (f, M, C, dt, (i + j) % 2 == 1)))
            out.append(("%s-long" % n, ("gauss",) + HEAD_LONG + (dt, False)))
            out.append(("%s-long" % n, ("quarter",) + HEAD_LONG + (dt, True)))
        elif kind == "ema" and dt == F32:
            for nn in EMA_N:
                for m in EMA_M:
                    for f in ("gauss", "integers"):
                        out.append(("n%d" % nn, (f, nn, m)))
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
                if n in BOUNDED and v > worst.get(n, 0.0):
                    worst[n] = v
                    log("k_ref %s = %.3f at %s %s %s" % (n, v, kind, grp, a[0]))
    return worst
