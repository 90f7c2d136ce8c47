"""Shared by the tests of the 3x3-convolution layer op (dpt_engine.Conv3x3Fn): the table of geometries whose kernel
choice is pinned, a recorder of the `ops` wrappers one forward + backward goes through, and the fp64 shifted-product
references.  The recorder uses only names and a signature that every version of the layer op has had, so the fixture
tests/golden/conv3x3_paths.json can be recorded on one commit and checked on the next."""
import contextlib
import json
import os

import torch

DEV = "cuda"
BF, F32, F64 = torch.bfloat16, torch.float32, torch.float64
FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "conv3x3_paths.json")

# (B, H, W, Cin, Cout, stride, dtype, bias, want_stats, relu_in): between them every branch of the choice
ROWS = [
    (2, 56, 56, 64, 64, 1, "bf16", False, True, True),       # 1  direct + statistics / direct / direct
    (4, 28, 28, 256, 256, 1, "bf16", False, True, False),    # 2  gather + statistics / gather / im2col
    (2, 56, 56, 128, 128, 2, "bf16", False, True, False),    # 3  gather + statistics / im2col / col2im
    (2, 56, 56, 96, 192, 2, "bf16", False, True, False),     # 4  im2col + statistics / im2col / col2im
    (2, 112, 112, 48, 96, 2, "bf16", False, True, False),    # 5  im2col + statistics / gather / col2im
    (1, 32, 32, 128, 32, 1, "bf16", True, False, False),     # 6  direct / direct / direct
    (8, 56, 56, 256, 256, 1, "bf16", True, False, True),     # 7  gather / gather / gather
    (1, 56, 56, 256, 256, 1, "bf16", True, False, False),    # 8  im2col / gather / im2col
    (2, 14, 14, 256, 256, 1, "bf16", True, False, False),    # 9  direct / im2col / direct
    (2, 56, 56, 96, 256, 1, "bf16", False, False, False),    # 10 direct / gather / direct
    (8, 28, 28, 192, 256, 1, "bf16", False, False, False),   # 11 im2col / gather / im2col
    (32, 28, 28, 192, 256, 1, "bf16", False, False, False),  # 12 gather / gather / gather
    (2, 14, 14, 768, 768, 2, "bf16", True, False, False),    # 13 im2col / im2col / col2im
    (4, 112, 112, 256, 128, 1, "bf16", True, False, False),  # 14 direct / direct / gather
    (25, 24, 24, 256, 512, 1, "bf16", True, False, False),   # 15 gather / gather / im2col
    (25, 24, 24, 512, 256, 1, "bf16", True, False, False),   # 16 im2col / gather / gather
    (1, 15, 17, 256, 256, 1, "bf16", True, False, False),    # 17 im2col / im2col / im2col
    (2, 56, 56, 64, 64, 1, "bf16", True, True, False),       # 18 bias and want_stats: no statistics
    (1, 8, 8, 64, 64, 1, "fp32", True, False, False),        # 19 im2col / im2col / im2col
    (1, 8, 8, 64, 64, 2, "fp32", False, True, False),        # 20 want_stats, but fp32: statistics come back None
]
DTYPES = {"bf16": BF, "fp32": F32}

WRAPPED = ("im2col3x3", "col2im3x3", "linear_fwd", "linear_bwd_data", "linear_bwd_weight", "conv3x3_fwd",
           "conv3x3_bwd_weight", "conv3x3_direct_fwd", "conv3x3_direct_wgrad", "conv3x3_wgrad_unpack", "relu_bwd",
           "colsum")
FLAGGED = ("conv3x3_fwd", "conv3x3_direct_fwd")   # recorded with colstats and `relu_mask is not None`


def flagged(name, colstats, masked):
    return f"{name}(colstats={bool(colstats)}, relu_mask={bool(masked)})"


@contextlib.contextmanager
def recording(log):
    """every call of an `ops` wrapper in WRAPPED appends its name to `log` and goes through"""
    from ssl4gie_amd import ops
    saved = {n: getattr(ops, n) for n in WRAPPED}

    def wrap(name, fn):
        def call(*a, **k):
            log.append(flagged(name, k.get("colstats", False), k.get("relu_mask") is not None)
                       if name in FLAGGED else name)
            return fn(*a, **k)
        return call
    try:
        for n, fn in saved.items():
            setattr(ops, n, wrap(n, fn))
        yield log
    finally:
        for n, fn in saved.items():
            setattr(ops, n, fn)


def ints(shape, seed, lo=-1, hi=2):
    """small integers drawn on the device (hundreds of millions of them: a host generator would take minutes)"""
    g = torch.Generator(DEV).manual_seed(seed)
    return torch.randint(lo, hi, shape, generator=g, device=DEV, dtype=torch.int8).to(BF)


def mm64(a, b):
    """fp64 product of two integer-valued bf16 matrices in row chunks (an [M, K] fp64 copy of a 800k-row operand
    would be gigabytes)"""
    out = torch.empty(a.shape[0], b.shape[1], dtype=F64, device=a.device)
    step = 1 << 18
    b64 = b.double()
    for i in range(0, a.shape[0], step):
        out[i:i + step] = a[i:i + step].double() @ b64
    return out


def conv_ref(x, w, stride):
    """x [B,H,W,Ci] (integer-valued bf16), w [Co,Ci,3,3] fp64 -> fp64 [B,Ho,Wo,Co], pad 1"""
    B, H, W, Ci = x.shape
    Co = w.shape[0]
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    xp = torch.zeros(B, H + 2, W + 2, Ci, dtype=BF, device=x.device)
    xp[:, 1:H + 1, 1:W + 1] = x
    out = torch.zeros(B * Ho * Wo, Co, dtype=F64, device=x.device)
    for dy in range(3):
        for dx in range(3):
            tap = xp[:, dy:dy + stride * (Ho - 1) + 1:stride, dx:dx + stride * (Wo - 1) + 1:stride].reshape(-1, Ci)
            out += mm64(tap, w[:, :, dy, dx].t().to(BF))
    return out.view(B, Ho, Wo, Co)


def conv_wgrad_ref(dy, x, stride):
    """dW[Co,Ci,3,3] fp64 = sum over output pixels of dy x patch"""
    B, H, W, Ci = x.shape
    _, Ho, Wo, Co = dy.shape
    xp = torch.zeros(B, H + 2, W + 2, Ci, dtype=BF, device=x.device)
    xp[:, 1:H + 1, 1:W + 1] = x
    dw = torch.zeros(Co, Ci, 3, 3, dtype=F64, device=x.device)
    d2 = dy.reshape(-1, Co)
    step = 1 << 18
    for ky in range(3):
        for kx in range(3):
            tap = xp[:, ky:ky + stride * (Ho - 1) + 1:stride, kx:kx + stride * (Wo - 1) + 1:stride].reshape(-1, Ci)
            acc = torch.zeros(Co, Ci, dtype=F64, device=x.device)
            for i in range(0, d2.shape[0], step):
                acc += d2[i:i + step].double().t() @ tap[i:i + step].double()
            dw[:, :, ky, kx] = acc
    return dw


def run_conv(row):
    """One Conv3x3Fn forward + backward on `row` with operands in {0, 1} x {-1, 0, 1} (every sum exact in fp32).
    -> (fwd, bwd, t): the wrappers called in forward and in backward, in order, and the tensors of the run"""
    from ssl4gie_amd.dpt_engine import Conv3x3Fn
    from ssl4gie_amd.engine import GradSink, LPCache
    B, H, W, Ci, Co, stride, dtype, bias, want_stats, relu_in = row
    dt = DTYPES[dtype]
    x = ints((B, H, W, Ci), 311, 0, 2).to(dt)
    w = ints((Co, Ci, 3, 3), 312).float()
    b = ints((Co,), 313, -2, 3).float() if bias else None
    xg = x.clone().requires_grad_(True)
    wg = w.clone().requires_grad_(True)
    bg = b.clone().requires_grad_(True) if bias else None
    fwd, bwd = [], []
    with recording(fwd):
        out = Conv3x3Fn.apply(xg, wg, bg, stride, relu_in, GradSink(None), LPCache(), want_stats)
    y, stats = out if want_stats else (out, None)
    dy = ints(tuple(y.shape), 314).to(dt)
    with recording(bwd):
        y.backward(dy)
        torch.cuda.synchronize()
    return fwd, bwd, dict(x=x, w=w, b=b, dy=dy, y=y.detach(), stats=stats, dx=xg.grad, dw=wg.grad,
                          db=bg.grad if bias else None)


def load_fixture():
    with open(FIXTURE) as f:
        return json.load(f)["rows"]
