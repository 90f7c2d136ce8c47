"""MoCo-v3 conv stem on the MI355X: (1) the 3-channel 3x3 stride-2 stem kernels against their byte floor, beside the
7x7 ResNet stem; (2) every stage of the ConvStem of vit_conv_base, forward and backward, at the training batch;
(3) one MoCo_ViT step on vit_conv_base beside the same step on vit_base.  python tools/convstem_bench.py [B]"""
import os
import sys
import time
from functools import partial

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

if not torch.cuda.is_available():
    sys.exit("convstem_bench: needs the GPU (there is no CPU path to measure)")
from ssl4gie_amd import ops  # noqa: E402
from ssl4gie_amd.conv_plan import conv3x3_plan  # noqa: E402
from ssl4gie_amd.engine import GradSink, LPCache, LinearFn  # noqa: E402
from ssl4gie_amd.dpt_engine import Conv3x3Fn  # noqa: E402
from ssl4gie_amd.resnet_engine import BatchNormFn, StemConv3x3Fn  # noqa: E402

B = int(sys.argv[1]) if len(sys.argv) > 1 else 256
BF = torch.bfloat16
PEAK = 8.0e12  # HBM3E bytes / s
H = W = 224
Ho = Wo = 112


def timeit(fn, fill=0.5):
    """us per call: device events around enough back-to-back calls to fill `fill` seconds, after a warm-up"""
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(5):
        fn()
    b.record()
    torch.cuda.synchronize()
    n = max(10, int(fill * 1e3 / max(a.elapsed_time(b) / 5, 1e-3)))
    a.record()
    for _ in range(n):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / n * 1e3


def line(name, us, nbytes):
    print(f"{name:34s} {us:8.1f} us   floor {nbytes / 1e6:7.1f} MB   {nbytes / us / 1e6:6.2f} TB/s   "
          f"{100 * nbytes / (us * 1e-6) / PEAK:5.1f} % of 8 TB/s", flush=True)


print(f"== 1. stem kernels, B = {B}, {H} x {W} (bytes = image read once + map written / read once)")
x = torch.randn(B, 3, H, W, device="cuda")
for C0 in (48, 96):
    w = torch.randn(C0, 3, 3, 3, device="cuda") * 0.2
    dy = torch.randn(B, Ho, Wo, C0, device="cuda").to(BF)
    floor = B * 3 * H * W * 4 + B * Ho * Wo * C0 * 2
    line(f"stem3x3_fwd  C0={C0} (+stats)", timeit(lambda: ops.stem3x3_fwd(x, w, BF, colstats=True)), floor)
    line(f"stem3x3_fwd  C0={C0}", timeit(lambda: ops.stem3x3_fwd(x, w, BF)), floor)
    line(f"stem3x3_wgrad C0={C0}", timeit(lambda: ops.stem3x3_wgrad(dy, x)), floor)
packed = ops.stem7x7_pack(x)
w7 = ops.stem7x7_weight(torch.randn(64, 3, 7, 7, device="cuda") * 0.05).to(BF)
dy7 = torch.randn(B, Ho, Wo, 64, device="cuda").to(BF)
floor7 = packed.numel() * 2 + B * Ho * Wo * 64 * 2
line("stem7x7_pack", timeit(lambda: ops.stem7x7_pack(x)), B * 3 * H * W * 4 + packed.numel() * 2)
line("stem7x7_fwd (+stats, packed image)", timeit(lambda: ops.stem7x7_fwd(packed, w7, B, H, W, colstats=True)), floor7)
line("stem7x7_wgrad (packed image)", timeit(lambda: ops.stem7x7_wgrad(dy7, packed, B, H, W)), floor7)
del packed, dy7

print(f"\n== 2. ConvStem(768) stage by stage at B = {B}, bf16 (each stage alone on its real input shape; backward = "
      "(forward + backward) - forward)")
sink, lp = GradSink(None), LPCache()
widths = [3, 96, 192, 384, 768]
res = [224, 112, 56, 28, 14]
tot_f = tot_b = 0.0
for i in range(4):
    cin, cout, hw = widths[i], widths[i + 1], res[i]
    conv = torch.nn.Conv2d(cin, cout, 3, 2, 1, bias=False).cuda()
    bn = torch.nn.BatchNorm2d(cout).cuda()
    gout = torch.randn(B, hw // 2, hw // 2, cout, device="cuda").to(BF)
    if i == 0:
        xin = x

        def fwd():
            y, st = StemConv3x3Fn.apply(xin, conv.weight, BF, sink, True)
            return BatchNormFn.apply(y, bn.weight, bn.bias, None, bn, True, sink, st, None)
    else:
        xin = torch.randn(B, hw, hw, cin, device="cuda").to(BF).requires_grad_(True)

        def fwd():
            y, st = Conv3x3Fn.apply(xin, conv.weight, None, 2, False, sink, lp, True)
            return BatchNormFn.apply(y, bn.weight, bn.bias, None, bn, True, sink, st, None)

    def fwd_only():
        with torch.no_grad():
            fwd()

    def fwd_bwd():
        conv.weight.grad = bn.weight.grad = bn.bias.grad = None
        if i:
            xin.grad = None
        fwd().backward(gout)

    tf, tfb = timeit(fwd_only, 0.3), timeit(fwd_bwd, 0.3)
    tot_f, tot_b = tot_f + tf, tot_b + tfb - tf
    kind = "direct stem kernels" if i == 0 else conv3x3_plan(B, hw, hw, cin, cout, 2, BF, False, True).fwd
    print(f"layer {i + 1}: {cin:3d} -> {cout:3d} @ {hw:3d}^2  conv + BatchNorm + ReLU   forward {tf:8.1f} us   backward "
          f"{tfb - tf:8.1f} us   ({kind})", flush=True)
    del xin, gout
lin = torch.nn.Conv2d(768, 768, 1).cuda()
xin = torch.randn(B * 196, 768, device="cuda").to(BF).requires_grad_(True)
gout = torch.randn(B * 196, 768, device="cuda").to(BF)


def pf():
    return LinearFn.apply(xin, lin.weight, lin.bias, BF, BF, sink, lp)


def pf_only():
    with torch.no_grad():
        pf()


def pfb():
    lin.weight.grad = lin.bias.grad = xin.grad = None
    pf().backward(gout)


tf, tfb = timeit(pf_only, 0.3), timeit(pfb, 0.3)
tot_f, tot_b = tot_f + tf, tot_b + tfb - tf
print(f"projection 768 -> 768 @ 14^2 (1x1, GEMM)                    forward {tf:8.1f} us   backward {tfb - tf:8.1f} us")
print(f"stem total                                                   forward {tot_f:8.1f} us   backward {tot_b:8.1f} us")
del xin, gout, x

print(f"\n== 3. MoCo_ViT step, two views of {B}, bf16, AdamW: vit_conv_base beside vit_base (alternated)")
from ssl4gie_amd.Models.moco_v3 import vits  # noqa: E402
from ssl4gie_amd.Models.moco_v3.moco import builder  # noqa: E402

g = torch.Generator().manual_seed(0)
x1 = torch.randn(B, 3, H, W, generator=g).cuda()
x2 = torch.randn(B, 3, H, W, generator=g).cuda()
models = {}
for name in ("vit_conv_base", "vit_base"):
    torch.manual_seed(0)
    m = builder.MoCo_ViT(partial(getattr(vits, name), stop_grad_conv1=True), 256, 4096, 0.2).cuda().set_precision("bf16")
    opt = torch.optim.AdamW([p for p in m.parameters() if p.requires_grad], lr=1e-4, fused=True)
    models[name] = (m, opt)


def step(name):
    m, opt = models[name]
    opt.zero_grad(set_to_none=True)
    loss = m(x1, x2, 0.99)
    loss.backward()
    opt.step()
    return loss


for name in models:
    for _ in range(3):
        step(name)
torch.cuda.synchronize()
ms = {k: [] for k in models}
host = {k: [] for k in models}
for rnd in range(3):
    for name in models:
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        a.record()
        step(name)                      # starts on an idle GPU: its host time is the pure enqueue cost
        host[name].append(1e3 * (time.perf_counter() - t0))
        for _ in range(4):
            loss = step(name)
        b.record()
        torch.cuda.synchronize()
        ms[name].append(a.elapsed_time(b) / 5)
        assert bool(torch.isfinite(loss)), name
for name in models:
    print(f"{name:14s} ms_per_step {sorted(ms[name])[1]:8.2f} (rounds {', '.join(f'{v:.2f}' for v in ms[name])})   "
          f"host_enqueue_ms {sorted(host[name])[1]:7.2f}")
