"""GPU: the kernels of csrc/atrous_ops.hip against fp64, per element.

Gate (the form of tests/test_gpu_det_heads.py): in fp32 mode max(2 d, 2^-20 max|want|), d = the largest error of torch's
own fp32 CPU op on the same inputs against fp64.  In bf16 the inputs are rounded to bf16 first (the references see the
rounded values) and every element gets the fp32 gate plus one bf16 rounding of the output, 2^-8 |want|.
"""
import functools

import pytest
import torch
import torch.nn.functional as F

from ssl4gie_amd import ops
from ssl4gie_amd.atrous_engine import DilatedConv3x3Fn
from ssl4gie_amd.engine import GradSink, LPCache

pytestmark = pytest.mark.gpu
DEV = "cuda"
DTYPES = [torch.float32, torch.bfloat16]


def _rn(shape, seed, dtype):
    """fp32 values that `dtype` holds exactly"""
    x = torch.randn(shape, generator=torch.Generator().manual_seed(seed))
    return x.to(dtype).float()


def _nhwc(x, dtype):
    return x.permute(0, 2, 3, 1).contiguous().to(dtype).to(DEV)


def _nchw(y):
    return y.detach().float().cpu().permute(0, 3, 1, 2).double()


def _check(name, got, want64, ref32, dtype, extra=0.0):
    """got: the kernel's result; want64 / ref32: the same op in fp64 / by torch in fp32 on the CPU"""
    d = float((ref32.double() - want64).abs().max())
    gate = max(2.0 * d, 2.0 ** -20 * float(want64.abs().max()))
    tol = torch.full_like(want64, gate) + extra
    if dtype == torch.bfloat16:
        tol = tol + 2.0 ** -8 * want64.abs()
    err = (got.double() - want64).abs()
    print(f"{name} [{str(dtype)[6:]}]: max err {float(err.max()):.3e}, torch fp32 distance {d:.3e}, gate {gate:.3e}")
    assert got.shape == want64.shape and bool((err <= tol).all()), (name, float((err - tol).max()))


# ------------------------------------------------------------------ dense dilated 3x3
@functools.lru_cache(maxsize=None)
def _dense_case(B, H, W, Cin, Cout, dil, dtype):
    x = _rn((B, Cin, H, W), 1, dtype)
    w = _rn((Cout, Cin, 3, 3), 2, dtype) / 8.0   # a power of two: still exact in bf16
    dy = _rn((B, Cout, H, W), 3, dtype)
    out = {}
    for tag, t in (("f64", torch.float64), ("f32", torch.float32)):
        xa, wa = x.clone().to(t).requires_grad_(True), w.clone().to(t).requires_grad_(True)
        y = F.conv2d(xa, wa, padding=dil, dilation=dil)
        y.backward(dy.to(t))
        out[tag] = (y.detach(), xa.grad, wa.grad)
    return x, w, dy, out


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("B,H,W,Cin,Cout,dil", [(2, 14, 14, 64, 64, 2), (1, 5, 7, 64, 128, 2), (1, 4, 4, 64, 64, 12)])
def test_dilated_conv3x3(B, H, W, Cin, Cout, dil, dtype):
    """forward, data gradient and weight gradient of DilatedConv3x3Fn (dilated patch matrix + the plain GEMMs): a square
    map, a non-square one smaller than two dilations, and a map on which only the centre tap is inside"""
    x, w, dy, ref = _dense_case(B, H, W, Cin, Cout, dil, dtype)
    xd = _nhwc(x, dtype).requires_grad_(True)
    wd = w.to(DEV).requires_grad_(True)
    y = DilatedConv3x3Fn.apply(xd, wd, dil, GradSink(None), LPCache())
    y.backward(_nhwc(dy, dtype))
    torch.cuda.synchronize()
    tag = f"dilated {B}x{H}x{W} {Cin}->{Cout} d={dil}"
    _check(tag + " fwd", _nchw(y), ref["f64"][0], ref["f32"][0], dtype)
    _check(tag + " dgrad", _nchw(xd.grad), ref["f64"][1], ref["f32"][1], dtype)
    _check(tag + " wgrad", wd.grad.cpu(), ref["f64"][2], ref["f32"][2], torch.float32)   # written in fp32 in both modes


def test_im2col3x3_dil_layout():
    """the matrix itself: dilation 1 is im2col3x3 bit for bit; pad columns are zero; taps outside the map are zero"""
    x = torch.randn(2, 5, 7, 8, device=DEV).bfloat16()
    assert torch.equal(ops.im2col3x3_dil(x, 1), ops.im2col3x3(x))
    cols = ops.im2col3x3_dil(x, 3).view(2, 5, 7, -1)
    assert cols.shape[-1] == 128 and float(cols[..., 72:].abs().max()) == 0.0
    want = F.pad(x.permute(0, 3, 1, 2).float(), (3, 3, 3, 3))
    for ky in range(3):
        for kx in range(3):
            tap = want[:, :, 3 * ky:3 * ky + 5, 3 * kx:3 * kx + 7].permute(0, 2, 3, 1)
            assert torch.equal(cols[..., (ky * 3 + kx) * 8:(ky * 3 + kx + 1) * 8].float(), tap), (ky, kx)


# ------------------------------------------------------------------ depthwise 3x3
@functools.lru_cache(maxsize=None)
def _dw_case(B, H, W, C, dil, dtype):
    x = _rn((B, C, H, W), 4, dtype)
    w = _rn((C, 1, 3, 3), 5, dtype)
    dy = _rn((B, C, H, W), 6, dtype)
    out = {}
    for tag, t in (("f64", torch.float64), ("f32", torch.float32)):
        xa, wa = x.to(t), w.clone().to(t).requires_grad_(True)
        y = F.conv2d(xa, wa, padding=dil, dilation=dil, groups=C)
        y.backward(dy.to(t))
        yf = F.conv2d(xa, wa.detach().flip(2, 3), padding=dil, dilation=dil, groups=C)
        out[tag] = (y.detach(), yf, wa.grad)
    return x, w, dy, out


DW_CASES = [(2, 14, 14, C, d) for C in (8, 304, 2048) for d in (1, 12, 24, 36)] + [(1, 3, 5, C, 1) for C in (8, 304, 2048)]


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("B,H,W,C,dil", DW_CASES)
def test_depthwise_conv3x3(B, H, W, C, dil, dtype):
    """forward, flipped forward (the data gradient) and weight gradient; rates 24 and 36 leave the centre tap alone on
    the 14 x 14 map.  The weight gradient repeats bit for bit, and `accumulate` adds to a pre-filled target (gate: one
    more fp32 addition, 2^-23 of the sum)"""
    x, w, dy, ref = _dw_case(B, H, W, C, dil, dtype)
    xd, dyd, wd = _nhwc(x, dtype), _nhwc(dy, dtype), w.to(DEV)
    tag = f"depthwise {B}x{H}x{W}x{C} d={dil}"
    _check(tag + " fwd", _nchw(ops.dwconv3x3_fwd(xd, wd, dil)), ref["f64"][0], ref["f32"][0], dtype)
    _check(tag + " flipped", _nchw(ops.dwconv3x3_fwd(xd, wd, dil, flip=True)), ref["f64"][1], ref["f32"][1], dtype)
    g1 = ops.dwconv3x3_wgrad(dyd, xd, dil)
    g2 = ops.dwconv3x3_wgrad(dyd, xd, dil)
    assert torch.equal(g1, g2)
    _check(tag + " wgrad", g1.cpu(), ref["f64"][2], ref["f32"][2], torch.float32)
    pre = torch.randn(C, 1, 3, 3, generator=torch.Generator().manual_seed(9))
    acc = pre.to(DEV)
    ops.dwconv3x3_wgrad(dyd, xd, dil, out=acc, accumulate=True)
    want = ref["f64"][2] + pre.double()
    _check(tag + " wgrad accumulate", acc.cpu(), want, ref["f32"][2] + pre, torch.float32, extra=2.0 ** -23 * want.abs())


# ------------------------------------------------------------------ bilinear x4, align_corners=True
@functools.lru_cache(maxsize=None)
def _up_case(B, H, W, C, dtype):
    x = _rn((B, C, H, W), 7, dtype)
    dy = _rn((B, C, 4 * H, 4 * W), 8, dtype)
    out = {}
    for tag, t in (("f64", torch.float64), ("f32", torch.float32)):
        xa = x.clone().to(t).requires_grad_(True)
        y = F.interpolate(xa, scale_factor=4, mode="bilinear", align_corners=True)
        y.backward(dy.to(t))
        out[tag] = (y.detach(), xa.grad)
    return x, dy, out


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("C", [1, 8, 256])
@pytest.mark.parametrize("B,H,W", [(2, 3, 5), (1, 14, 14)])
def test_bilinear_up_ac(B, H, W, C, dtype):
    """forward against F.interpolate(scale_factor=4, mode="bilinear", align_corners=True), backward against its
    autograd; C = 1 (the logit map) takes the element-wise path, 8 and 256 the 16-byte one"""
    x, dy, ref = _up_case(B, H, W, C, dtype)
    tag = f"up x4 {B}x{H}x{W}x{C}"
    _check(tag + " fwd", _nchw(ops.bilinear_up_ac_fwd(_nhwc(x, dtype), 4)), ref["f64"][0], ref["f32"][0], dtype)
    _check(tag + " bwd", _nchw(ops.bilinear_up_ac_bwd(_nhwc(dy, dtype), 4)), ref["f64"][1], ref["f32"][1], dtype)


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
def test_bilinear_up_ac_single_pixel(dtype):
    """a 1 x 1 input: (H - 1) / (sH - 1) = 0, the map is the constant; its gradient is the sum over the map"""
    x = _rn((2, 1, 1, 8), 10, dtype).to(dtype).to(DEV)
    y = ops.bilinear_up_ac_fwd(x, 4)
    assert y.shape == (2, 4, 4, 8) and torch.equal(y, x.expand(2, 4, 4, 8))
    dy = _rn((2, 4, 4, 8), 11, dtype)
    got = ops.bilinear_up_ac_bwd(dy.to(dtype).to(DEV), 4).float().cpu().double()
    want = dy.double().sum((1, 2), keepdim=True)
    tol = 16 * 2.0 ** -24 * dy.double().abs().sum((1, 2), keepdim=True) + (2.0 ** -8 * want.abs() if dtype == torch.bfloat16 else 0)
    assert bool(((got - want).abs() <= tol).all())


def test_chan_copy_concatenates_and_broadcasts():
    """the concatenation helper: slices written side by side (a [B, C] part over every pixel) and read back, bit for bit"""
    a = torch.randn(2, 3, 5, 256, device=DEV).bfloat16()
    b = torch.randn(2, 3, 5, 48, device=DEV).bfloat16()
    p = torch.randn(2, 8, device=DEV).bfloat16()
    out = torch.empty(2, 3, 5, 312, device=DEV, dtype=torch.bfloat16)
    ops.chan_write(out, 0, a), ops.chan_write(out, 256, b), ops.chan_write(out, 304, p)
    assert torch.equal(out, torch.cat([a, b, p.view(2, 1, 1, 8).expand(2, 3, 5, 8)], dim=-1))
    assert torch.equal(ops.chan_read(out, 256, 48), b)
    f = torch.randn(2, 3, 5, 8, device=DEV)
    assert torch.equal(ops.chan_read(f, 3, 1), f[..., 3:4])   # a width that is no 16-byte chunk
