"""GPU: the MAE fine-tuning recipe on the engine (reference Models/mae/main_finetune.py) — stochastic depth in the
native block executor, the Mixup kernels, the soft-target / label-smoothing cross-entropy and one end-to-end step of
the `models_vit` classifier — against the fp64 restatements of tests/finetune_checks.py.

Bars.  Block against fp64, measured as tests/test_gpu_blocks_well_conditioned.py measures it (relative L2 of the
output and the input gradient, worst parameter gradient relative to the largest of its kind): fp32 1e-3, the
project's bar; bf16 1.5 x the errors of the EXISTING no-drop path on the same block and inputs, and not below that
file's BF16_MEASURED["block197"].  Measured on an MI355X (profiles/finetune_recipe_timing.log):
    block 5x197x768  bf16  no drop: out 1.966e-03 dx 2.879e-03 param 4.267e-03
                           drop:    out 1.759e-03 dx 2.575e-03 param 3.920e-03
    block 5x197x768  fp32  no drop: out 6.371e-07 dx 6.995e-07 param 8.521e-07
                           drop:    out 5.722e-07 dx 6.257e-07 param 8.429e-07
    block 2x197x1024 fp32  drop:    out 6.441e-07 dx 6.534e-07 param 7.368e-07
    end to end (fp32): logits 4.4e-07, loss 8.6e-09, worst parameter gradient 6.4e-07
Dropped samples, the unchanged paths, the Mixup kernels and run-to-run results are compared bit for bit.  Losses:
max(1e-5, 8 e32), the rule of tests/test_gpu_loss_heads.py (e32: the error of torch's CPU fp32 formulation on the same
inputs).  End to end: 1e-3 in fp32; the AdamW step 1e-5, the bar of tests/test_gpu_optim.py."""
import argparse
import ctypes as C
import functools
from functools import partial

import numpy as np
import pytest
import torch

import finetune_checks as fc
from conftest import keyed_weights, rel_err
from test_gpu_blocks_well_conditioned import BF16_MEASURED, _param_errors, l2

pytestmark = pytest.mark.gpu
DEV = "cuda"
KEEP = 0.9


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from ssl4gie_amd import _lib
    _lib.load()


def G(seed):
    return torch.Generator("cpu").manual_seed(seed)


def _bar(e32):
    return max(1e-5, 8.0 * e32)


def _scalar_err(a, b):
    a, b = float(a.detach() if torch.is_tensor(a) else a), float(b)
    return abs(a - b) / (abs(b) if b != 0 else 1.0)


# ---------------------------------------------------------------------------------------------- one native block
_NAMES = ("ln1_g", "ln1_b", "wqkv", "bqkv", "wproj", "bproj", "ln2_g", "ln2_b", "wfc1", "bfc1", "wfc2", "bfc2")


def _native_block(blk, x, dy, prec, s_attn=None, s_mlp=None, dp=True, poison=False):
    """ssl4gie_block_fwd[_dp] + ssl4gie_block_bwd[_dp] on one Block, called directly -> (x_out, dx_in, grads) on the
    CPU.  poison: the whole workspace holds +inf before either call (every slot is written before it is read)."""
    from ssl4gie_amd import _lib, engine, ops
    L = _lib.load()
    dt = torch.float32 if prec == "fp32" else torch.bfloat16
    B, N, D = x.shape
    params = engine._block_params(blk)
    cfg = engine.StackCfg(heads=blk.num_heads, eps=blk.norm1.eps, dtype=dt, taps=(), need_bwd=True,
                          sink=engine.GradSink(None), lp=engine._GLOBAL_LP)
    w, keep = engine._weights_struct(params, cfg)
    F_ = params[8].shape[0]
    dims = _lib.BlockDims(B, N, D, blk.num_heads, F_, ops.code(dt), float(blk.norm1.eps))
    wsb = (L.ssl4gie_block_dp_workspace_bytes if dp else L.ssl4gie_block_workspace_bytes)(C.byref(dims))
    assert wsb > 0 and wsb % 4 == 0
    ws = torch.full((wsb // 4,), float("inf") if poison else 0.0, dtype=torch.float32, device=DEV)
    layout = engine._ActArena(B, N, D, blk.num_heads, F_, 2 if dt == torch.bfloat16 else 4)
    acts = torch.empty(layout.total, dtype=torch.uint8, device=DEV)
    a = layout.struct(acts.data_ptr())
    st = ops.stream()
    xo = torch.empty_like(x)
    sa, sm = ops.ptr(s_attn), ops.ptr(s_mlp)
    if dp:
        _lib.check(L.ssl4gie_block_fwd_dp(C.byref(dims), C.byref(w), C.byref(a), x.data_ptr(), xo.data_ptr(), sa, sm,
                                          ws.data_ptr(), st), "block_fwd_dp")
    else:
        assert s_attn is None and s_mlp is None
        _lib.check(L.ssl4gie_block_fwd(C.byref(dims), C.byref(w), C.byref(a), x.data_ptr(), xo.data_ptr(),
                                       ws.data_ptr(), st), "block_fwd")
    if poison:
        ws.fill_(float("inf"))
    grads = [torch.empty_like(p) for p in params]
    g = _lib.BlockGrads()
    for name, t in zip(_NAMES, grads):
        setattr(g, name, t.data_ptr())
    dy_lp = ops.cast(dy, dt) if dt != torch.float32 else None
    dx = torch.empty_like(x)
    dx_lp = torch.empty(x.shape, dtype=dt, device=DEV) if dt != torch.float32 else None
    head = (C.byref(dims), C.byref(w), C.byref(a), C.byref(g), x.data_ptr(), dy.data_ptr(), ops.ptr(dy_lp),
            dx.data_ptr(), ops.ptr(dx_lp))
    if dp:
        _lib.check(L.ssl4gie_block_bwd_dp(*head, sa, sm, 0, ws.data_ptr(), st), "block_bwd_dp")
    else:
        _lib.check(L.ssl4gie_block_bwd(*head, 0, ws.data_ptr(), st), "block_bwd")
    torch.cuda.synchronize()
    del keep
    return xo.cpu(), dx.cpu(), [t.cpu() for t in grads]


@functools.lru_cache(maxsize=None)
def _block197():
    """block 3 of the ViT-B trunk with the keyed weights of tests/test_gpu_blocks_well_conditioned.py, B = 5 (an odd
    batch on the half-tail attention tile), and its fp64 results without and with the fixed tables: sample 0 dropped
    in the attention branch only, 1 in the MLP branch only, 2 in both, 3 and 4 in neither"""
    from ssl4gie_amd.Models import models
    g = G(203)
    m = models.ViT_from_MAE(None, True, 6, False, None, False, None, 768, 12, 12, "cls")
    keyed_weights(m, 55, keep=("pos_embed", "decoder_pos_embed"))
    blk, pre = m.blocks[3], "blocks.3."
    sd = {k: v.detach().clone().double() for k, v in m.state_dict().items() if k.startswith(pre)}
    x = torch.randn(5, 197, 768, generator=g)
    dy = torch.randn(5, 197, 768, generator=g)
    k = 1.0 / KEEP
    s_attn = torch.tensor([0.0, k, 0.0, k, k])
    s_mlp = torch.tensor([k, 0.0, 0.0, k, k])
    ref = {}
    for tag, sa, sm in (("plain", None, None), ("drop", s_attn, s_mlp)):
        sdr = {kk: v.clone().requires_grad_(True) for kk, v in sd.items()}
        xr = x.double().requires_grad_(True)
        yr = fc.block(sdr, pre, xr, 12, m.norm.eps, sa, sm)
        yr.backward(dy.double())
        ref[tag] = (yr.detach(), xr.grad, {kk: v.grad for kk, v in sdr.items()})
    blk.to(DEV)
    return blk, pre, x, dy, s_attn, s_mlp, ref


@functools.lru_cache(maxsize=None)
def _run197(prec, which, poison=False):
    blk, pre, x, dy, s_attn, s_mlp, _ = _block197()
    xd, dyd = x.to(DEV), dy.to(DEV)
    if which == "plain":
        return _native_block(blk, xd, dyd, prec, dp=False)
    if which == "null":
        return _native_block(blk, xd, dyd, prec, dp=True)
    return _native_block(blk, xd, dyd, prec, s_attn.to(DEV), s_mlp.to(DEV), dp=True, poison=poison)


_PARAM_NAMES = ("norm1.weight", "norm1.bias", "attn.qkv.weight", "attn.qkv.bias", "attn.proj.weight", "attn.proj.bias",
                "norm2.weight", "norm2.bias", "mlp.fc1.weight", "mlp.fc1.bias", "mlp.fc2.weight", "mlp.fc2.bias")


def _errors(run, ref, pre):
    """the three errors of test_gpu_blocks_well_conditioned.py: output, input gradient, worst parameter gradient"""
    xo, dx, grads = run
    yr, dxr, gr = ref
    named = [(pre + n, argparse.Namespace(grad=t)) for n, t in zip(_PARAM_NAMES, grads)]
    e_p, where = _param_errors(named, gr)
    return {"out": l2(xo, yr), "dx": l2(dx, dxr), "param": e_p}, where


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_dropped_sample_identities(prec):
    blk, pre, x, dy, s_attn, s_mlp, _ = _block197()
    xo, dx, grads = _run197(prec, "drop")
    # the sample dropped in both branches passes through bit for bit, forward and backward
    assert torch.equal(xo[2], x[2])
    assert torch.equal(dx[2], dy[2])
    # the others do not
    for b in (0, 1, 3, 4):
        assert not torch.equal(xo[b], x[b]) and not torch.equal(dx[b], dy[b])
    # the same with +inf in every workspace slot (the branch scratch included) before either call, and run to run
    xo2, dx2, grads2 = _run197(prec, "drop", poison=True)
    assert torch.equal(xo2[2], x[2]) and torch.equal(dx2[2], dy[2])
    assert torch.equal(xo, xo2) and torch.equal(dx, dx2)
    assert all(torch.equal(a, b) for a, b in zip(grads, grads2))
    assert all(bool(torch.isfinite(t).all()) for t in [xo2, dx2] + grads2)


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_drop_path_kernels_never_read_a_dropped_sample(prec):
    """ssl4gie_drop_path_add / _scale_cast directly: the dropped sample's branch values are +inf / NaN"""
    from ssl4gie_amd import _lib, ops
    L = _lib.load()
    g = G(7)
    B, per = 5, 197 * 768
    res, t, dx = (torch.randn(B, per, generator=g).to(DEV) for _ in range(3))
    s = torch.tensor([1 / KEEP, 0.0, 1 / KEEP, 0.0, 1.0], device=DEV)
    t[1], t[3] = float("inf"), float("nan")
    dx[1], dx[3] = float("inf"), float("nan")
    out = torch.empty_like(res)
    _lib.check(L.ssl4gie_drop_path_add(res.data_ptr(), t.data_ptr(), s.data_ptr(), out.data_ptr(), B, per,
                                       ops.stream()), "drop_path_add")
    assert torch.equal(out[1], res[1]) and torch.equal(out[3], res[3])
    want = res.double() + s.double().view(B, 1) * torch.where(torch.isfinite(t), t, torch.zeros_like(t)).double()
    assert float((out.double() - want)[[0, 2, 4]].abs().max()) < 1e-6
    dt = torch.float32 if prec == "fp32" else torch.bfloat16
    ys = torch.full((B, per), float("nan"), dtype=dt, device=DEV)
    _lib.check(L.ssl4gie_drop_path_scale_cast(dx.data_ptr(), s.data_ptr(), ys.data_ptr(), ops.code(dt), B, per,
                                              ops.stream()), "drop_path_scale_cast")
    assert float(ys[1].abs().max()) == 0.0 and float(ys[3].abs().max()) == 0.0
    assert torch.equal(ys[[0, 2, 4]], (dx[[0, 2, 4]] * s[[0, 2, 4]].view(3, 1)).to(dt))
    # a sample size that is no multiple of the vector: refused
    assert L.ssl4gie_drop_path_add(res.data_ptr(), t.data_ptr(), s.data_ptr(), out.data_ptr(), B, per - 2,
                                   ops.stream()) == 1000


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_drop_path_block_vs_fp64(prec):
    blk, pre, x, dy, s_attn, s_mlp, ref = _block197()
    e_plain, _ = _errors(_run197(prec, "plain"), ref["plain"], pre)
    e_drop, where = _errors(_run197(prec, "drop"), ref["drop"], pre)
    print(f"block 5x197x768 [{prec}] no drop: out {e_plain['out']:.3e} dx {e_plain['dx']:.3e} param {e_plain['param']:.3e}")
    print(f"block 5x197x768 [{prec}] drop:    out {e_drop['out']:.3e} dx {e_drop['dx']:.3e} param {e_drop['param']:.3e} ({where})")
    for k in ("out", "dx", "param"):
        bar = 1e-3 if prec == "fp32" else max(1.5 * e_plain[k], BF16_MEASURED["block197"][k])
        assert e_drop[k] < bar, (k, e_drop[k], bar, where)


def test_null_tables_are_the_plain_block():
    """ssl4gie_block_{fwd,bwd}_dp with both tables NULL against ssl4gie_block_{fwd,bwd}: bit for bit"""
    for prec in ("fp32", "bf16"):
        a, b = _run197(prec, "plain"), _run197(prec, "null")
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
        assert all(torch.equal(p, q) for p, q in zip(a[2], b[2]))


def test_vit_large_block_fp32():
    """D = 1024, H = 16: the block shape of vit_large_patch16"""
    from ssl4gie_amd.Models.vit_layers import Block
    g = G(31)
    blk = Block(1024, 16, norm_layer=partial(torch.nn.LayerNorm, eps=1e-6))
    with torch.no_grad():
        for n, p in blk.named_parameters():
            if p.ndim > 1:
                p.copy_(torch.randn(p.shape, generator=g) * 0.02)
            elif "norm" in n and n.endswith("weight"):
                p.copy_(1.0 + 0.1 * torch.randn(p.shape, generator=g))
            else:
                p.copy_(0.1 * torch.randn(p.shape, generator=g))
    pre = "b."
    x = torch.randn(2, 197, 1024, generator=g)
    dy = torch.randn(2, 197, 1024, generator=g)
    s_attn, s_mlp = torch.tensor([1 / KEEP, 0.0]), torch.tensor([1 / KEEP, 1 / KEEP])
    sdr = {pre + k: v.detach().clone().double().requires_grad_(True) for k, v in blk.state_dict().items()}
    xr = x.double().requires_grad_(True)
    yr = fc.block(sdr, pre, xr, 16, 1e-6, s_attn, s_mlp)
    yr.backward(dy.double())
    blk.to(DEV)
    run = _native_block(blk, x.to(DEV), dy.to(DEV), "fp32", s_attn.to(DEV), s_mlp.to(DEV))
    e, where = _errors(run, (yr.detach(), xr.grad, {k: v.grad for k, v in sdr.items()}), pre)
    print(f"block 2x197x1024 [fp32] drop: out {e['out']:.3e} dx {e['dx']:.3e} param {e['param']:.3e} ({where})")
    assert e["out"] < 1e-3 and e["dx"] < 1e-3 and e["param"] < 1e-3, (e, where)


# ---------------------------------------------------------------------------------------------- the stack in Python
def _small_vit(rate, seed=5):
    from ssl4gie_amd.Models.mae import models_vit
    torch.manual_seed(seed)
    m = models_vit.VisionTransformer(img_size=64, embed_dim=192, depth=3, num_heads=3, num_classes=10,
                                     global_pool=True, drop_path_rate=rate)
    g = G(seed)
    with torch.no_grad():   # biases and affine tables away from their zero / one initialisation
        for n, p in m.named_parameters():
            if p.ndim == 1:
                p.add_(0.1 * torch.randn(p.shape, generator=g))
    return m


def _step(m, imgs, w, **kw):
    for p in m.parameters():
        p.grad = None
    out = m(imgs, **kw)
    (out * w).sum().backward()
    torch.cuda.synchronize()
    return out.detach().clone(), {n: p.grad.detach().clone() for n, p in m.named_parameters()}


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_unchanged_paths_are_bit_equal(prec):
    g = G(41)
    imgs = torch.randn(6, 3, 64, 64, generator=g).to(DEV)
    w = torch.randn(6, 10, generator=g).to(DEV)
    base = _small_vit(0.0).to(DEV).set_precision(prec)
    out0, g0 = _step(base, imgs, w)
    # rates > 0 in eval(): the stack as it always ran
    m = _small_vit(0.5).to(DEV).set_precision(prec)
    assert [b.drop_path for b in m.blocks] == [0.0, 0.25, 0.5]
    m.eval()
    out1, g1 = _step(m, imgs, w)
    assert torch.equal(out0, out1) and all(torch.equal(g0[n], g1[n]) for n in g0)
    # training mode without gradients: nothing is drawn either
    m.train()
    with torch.no_grad():
        assert torch.equal(m(imgs), out0)
    # training mode with gradients: the factors are drawn, samples are dropped
    out2, g2 = _step(m, imgs, w)
    assert not torch.equal(out2, out0) and bool(torch.isfinite(out2).all())
    assert all(bool(torch.isfinite(v).all()) for v in g2.values())
    # all-ones tables run the scaled path: equal to the plain one within rounding, not bit for bit required
    ones = torch.ones(3, 2, 6, device=DEV)
    out3, g3 = _step(m, imgs, w, drop_scales=ones)
    assert rel_err(out3, out0) < (1e-5 if prec == "fp32" else 3e-2)


def test_bf16_stack_with_fixed_scales_follows_fp32():
    """the Python stack (two-workspace ring, tables on some blocks only) in bf16 against the same stack in fp32, at the
    bars of smoke() for this pair of precisions: 3e-2 on the output, 0.1 on a weight gradient"""
    g = G(43)
    imgs = torch.randn(6, 3, 64, 64, generator=g).to(DEV)
    w = torch.randn(6, 10, generator=g).to(DEV)
    k1, k2 = 1.0 / 0.75, 2.0
    scales = torch.tensor([[[1, 1, 1, 1, 1, 1], [1, 1, 1, 1, 1, 1]],
                           [[k1, 0, k1, k1, 0, k1], [k1, k1, 0, k1, 0, k1]],
                           [[k2, k2, 0, 0, 0, k2], [0, k2, k2, 0, 0, k2]]], dtype=torch.float32, device=DEV)
    res = {}
    for prec in ("fp32", "bf16"):
        m = _small_vit(0.5).to(DEV).set_precision(prec)
        with torch.no_grad():
            m.head.weight.mul_(10.0)
        res[prec] = _step(m, imgs, w, drop_scales=scales)
    assert rel_err(res["bf16"][0], res["fp32"][0]) < 3e-2
    for n in ("head.weight", "blocks.0.attn.qkv.weight", "blocks.2.mlp.fc2.weight", "patch_embed.proj.weight"):
        assert rel_err(res["bf16"][1][n], res["fp32"][1][n]) < 0.1, n
    # sample 4 is dropped everywhere from block 1 on: its logits are those of a one-block model, in both precisions
    assert bool(torch.isfinite(res["bf16"][0]).all())


def test_drawn_scales_follow_the_schedule():
    from ssl4gie_amd import engine
    depth, B, rate = 12, 4096, 0.1
    rates = fc.linspace_rates(rate, depth)
    s = engine.draw_drop_scales(rates, B, torch.device(DEV))
    assert s.dtype == torch.float32 and tuple(s.shape) == (depth, 2, B) and s.is_contiguous() and s.is_cuda
    s2 = engine.draw_drop_scales(rates, B, torch.device(DEV))
    assert not torch.equal(s, s2)
    s = s.cpu()
    for i, r in enumerate(rates):
        keep = np.float32(1.0 - r)
        vals = set(np.unique(s[i].numpy()).tolist())
        assert vals <= {0.0, float(np.float32(1.0) / keep)}, (i, vals)
        share = float((s[i] != 0).double().mean())
        assert abs(share - (1.0 - r)) <= fc.five_sigma(1.0 - r, 2 * B) + 1e-12, (i, share)
    assert float(s[0].min()) == 1.0   # rate 0: never dropped


# ---------------------------------------------------------------------------------------------- Mixup
def _mix_tables(B, H, W, variant):
    lam = torch.tensor([0.3, 0.9, 0.55, 0.25, 0.71, 1.0])[:B].clone()
    use = torch.tensor([0, 1, 1, 1, 0, 1], dtype=torch.uint8)[:B].clone()
    if variant == 0:    # blend | full image | top-left corner | bottom-right corner | blend | empty box
        box = [[0, 0, 0, 0], [0, H, 0, W], [0, 5, 0, 7], [H - 3, H, W - 5, W], [0, 0, 0, 0], [0, 0, 0, 0]]
    elif variant == 1:  # left border, full height | right border, one column | top rows | bottom row | interior, odd
        box = [[0, 0, 0, 0], [0, H, 0, 3], [2, H - 2, W - 1, W], [0, 2, 0, W], [0, 0, 0, 0], [H - 1, H, 1, W - 1]]
        use[4] = 1
        box[4] = [5, 14, 3, 10]
    elif variant == 2:  # mixup only, a distinct lambda per sample
        use.zero_()
        box = [[0, 0, 0, 0]] * 6
    else:               # cutmix only, interior boxes that cut through 16-byte vectors
        use.fill_(1)
        box = [[1, 9, 1, 6], [3, 4, 5, 6], [0, H, 2, W - 3], [7, 20, 9, 27], [4, 4, 1, 9], [2, 11, 6, 6]]
    box = torch.tensor(box, dtype=torch.int32)[:B].clone()
    area = ((box[:, 1] - box[:, 0]) * (box[:, 3] - box[:, 2])).double()
    lam = torch.where(use != 0, (1.0 - area / (H * W)).float(), lam)
    return lam, box, use


@pytest.mark.parametrize("variant", [0, 1, 2, 3])
@pytest.mark.parametrize("HW", [32, 30])
@pytest.mark.parametrize("B", [6, 5])
def test_mixup_kernel_bit_for_bit(B, HW, variant):
    from ssl4gie_amd import data, ops
    g = G(1000 * B + 10 * HW + variant)
    x = torch.randn(B, 3, HW, HW, generator=g)
    y = torch.randint(0, 10, (B,), generator=g)
    lam, box, use = _mix_tables(B, HW, HW, variant)
    xd = x.to(DEV)
    want = data.mixup_torch(xd.clone(), lam.to(DEV), box.to(DEV), use.to(DEV))   # out of place, on a clone
    got = ops.mixup(xd, lam.to(DEV), box.to(DEV), use.to(DEV))
    assert got is xd   # in place
    assert torch.equal(got.view(torch.int32), want.view(torch.int32))
    assert torch.equal(got.cpu(), fc.mixup_images(x, lam, box, use))   # ... and the sample-by-sample statement in fp32
    st = ops.mixup_target(y.to(DEV), lam.to(DEV), 10, 0.1)
    assert torch.equal(st, data.mixup_target_torch(y.to(DEV), lam.to(DEV), 10, 0.1))
    assert rel_err(st, fc.mixup_targets(y, lam, 10, 0.1)) < 1e-6


def test_mixup_refuses_bad_tables_in_bounds():
    """a box outside the image, a NaN lambda, a label outside [0, C): NaN samples / rows, nothing else touched"""
    from ssl4gie_amd import ops
    g = G(3)
    B, H, W, guard = 4, 30, 30, 4096
    buf = torch.randn(guard + B * 3 * H * W + guard, generator=g).to(DEV)
    before = buf.clone()
    x = buf[guard:guard + B * 3 * H * W].view(B, 3, H, W)
    lam = torch.tensor([0.5, float("nan"), 0.5, 0.5], device=DEV)
    box = torch.tensor([[0, H + 5, 0, W], [0, 0, 0, 0], [0, 0, 0, 0], [-1, 4, 2, 1 << 30]], dtype=torch.int32, device=DEV)
    use = torch.tensor([1, 0, 0, 1], dtype=torch.uint8, device=DEV)
    ops.mixup(x, lam, box, use)
    torch.cuda.synchronize()
    assert bool(torch.isnan(x[0]).all()) and bool(torch.isnan(x[1]).all()) and bool(torch.isnan(x[3]).all())
    want2 = before[guard:guard + B * 3 * H * W].view(B, 3, H, W)
    assert torch.equal(x[2], want2[2] * 0.5 + want2[1] * 0.5)
    assert torch.equal(buf[:guard], before[:guard]) and torch.equal(buf[-guard:], before[-guard:])
    y = torch.tensor([1, 10, -1, 3], device=DEV)
    st = ops.mixup_target(y, torch.full((4,), 0.5, device=DEV), 10, 0.1)
    assert bool(torch.isnan(st[1]).all()) and bool(torch.isnan(st[2]).all())   # rows 1 and 2 pair up: both labels are bad
    assert bool(torch.isfinite(st[0]).all()) and bool(torch.isfinite(st[3]).all())
    with pytest.raises(ValueError):
        ops.mixup(x, lam, box.to(torch.int64), use)


@pytest.mark.parametrize("mode", ["batch", "pair", "elem"])
def test_mixup_class_on_device_matches_its_cpu_formulation(mode):
    from ssl4gie_amd.data import Mixup
    g = G(17)
    kw = dict(mixup_alpha=0.8, cutmix_alpha=1.0, mode=mode, label_smoothing=0.1, num_classes=10)
    dev_mix, cpu_mix = Mixup(rng=np.random.RandomState(4), **kw), Mixup(rng=np.random.RandomState(4), **kw)
    for _ in range(3):   # three calls: the staging buffers are used in turn
        x = torch.randn(6, 3, 32, 32, generator=g)
        y = torch.randint(0, 10, (6,), generator=g)
        xd = x.to(DEV)
        got, st = dev_mix(xd, y.to(DEV))
        want, st_cpu = cpu_mix(x.clone(), y)
        assert got is xd and torch.equal(got.cpu(), want) and torch.equal(st.cpu(), st_cpu)


# ---------------------------------------------------------------------------------------------- losses
SHAPES = [(1, 1), (5, 6), (5, 1000), (3, 1003)]
CASES = ["plain", "pm80", "unnormalised"]


@functools.lru_cache(maxsize=None)
def _loss_case(B, Cn, case):
    g = G(10 * B + Cn + len(case))
    x = torch.randn(B, Cn, generator=g) * 3
    if case == "pm80":
        x = torch.where(torch.rand(B, Cn, generator=g) < 0.5, -80.0, 80.0) + 0.01 * torch.randn(B, Cn, generator=g)
    t = torch.rand(B, Cn, generator=g)
    t = t * 2.0 if case == "unnormalised" else t / t.sum(1, keepdim=True)
    y = torch.randint(0, Cn, (B,), generator=g)
    return x, t, y


def _check_loss(mod, ref, x, arg):
    l64, d64 = fc.loss_and_grad(ref, x, arg)
    l32, d32 = fc.loss_and_grad(ref, x, arg, dtype=torch.float32)
    bar_l, bar_d = _bar(_scalar_err(l32, l64)), _bar(rel_err(d32, d64))
    runs = []
    for _ in range(2):
        xd = x.to(DEV).requires_grad_(True)
        loss = mod(xd, arg.to(DEV))
        assert loss.grad_fn is not None and type(loss.grad_fn).__name__.startswith("_SoftCeFn")   # the fused path
        loss.backward()
        runs.append((loss.detach().cpu(), xd.grad.cpu()))
    el, ed = _scalar_err(runs[0][0], l64), rel_err(runs[0][1], d64)
    print(f"{type(mod).__name__} {tuple(x.shape)}: loss err {el:.2e} (bar {bar_l:.2e}), dlogits err {ed:.2e} (bar {bar_d:.2e})")
    assert el < bar_l and ed < bar_d
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])   # run to run


@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("B,Cn", SHAPES)
def test_soft_target_ce_vs_fp64(B, Cn, case):
    from ssl4gie_amd.losses import SoftTargetCrossEntropy
    x, t, _ = _loss_case(B, Cn, case)
    _check_loss(SoftTargetCrossEntropy(), fc.soft_target_ce, x, t)


@pytest.mark.parametrize("case", CASES[:2])
@pytest.mark.parametrize("B,Cn", SHAPES)
def test_label_smoothing_ce_vs_fp64(B, Cn, case):
    from ssl4gie_amd.losses import LabelSmoothingCrossEntropy
    x, _, y = _loss_case(B, Cn, case)
    _check_loss(LabelSmoothingCrossEntropy(0.1), lambda a, b: fc.label_smoothing_ce(a, b, 0.1), x, y)


@pytest.mark.parametrize("B,Cn", SHAPES[1:])
def test_soft_losses_bf16_logits(B, Cn):
    """bf16 logits are read as the fp32 values they hold; the gradient is the fp32 kernel's, rounded once"""
    from ssl4gie_amd.losses import LabelSmoothingCrossEntropy, SoftTargetCrossEntropy
    x, t, y = _loss_case(B, Cn, "plain")
    xb = x.to(torch.bfloat16)
    for mod, arg, ref in ((SoftTargetCrossEntropy(), t, fc.soft_target_ce),
                          (LabelSmoothingCrossEntropy(0.1), y, lambda a, b: fc.label_smoothing_ce(a, b, 0.1))):
        l64, d64 = fc.loss_and_grad(ref, xb.float(), arg)
        l32, d32 = fc.loss_and_grad(ref, xb.float(), arg, dtype=torch.float32)
        xd = xb.to(DEV).requires_grad_(True)
        loss = mod(xd, arg.to(DEV))
        loss.backward()
        xf = xb.float().to(DEV).requires_grad_(True)
        loss_f = mod(xf, arg.to(DEV))
        loss_f.backward()
        assert loss.dtype == torch.float32 and xd.grad.dtype == torch.bfloat16
        assert _scalar_err(loss, l64) < _bar(_scalar_err(l32, l64))
        assert rel_err(xf.grad, d64) < _bar(rel_err(d32, d64))
        assert torch.equal(loss, loss_f) and torch.equal(xd.grad, xf.grad.to(torch.bfloat16))


def test_label_out_of_range_is_nan_and_stays_in_bounds():
    from ssl4gie_amd import _lib
    L = _lib.load()
    B, Cn, guard = 9, 6, 64
    g = G(5)
    x = torch.randn(B, Cn, generator=g).to(DEV)
    for bad in (Cn, -1, 1 << 40):
        t = torch.randint(0, Cn, (B,), generator=g)
        t[4] = bad
        t = t.to(DEV)
        buf = torch.full((guard + B * Cn + guard,), 7.0, device=DEV)
        loss = torch.zeros((), device=DEV)
        ws = torch.zeros(L.ssl4gie_soft_cross_entropy_workspace_bytes(B, Cn), dtype=torch.uint8, device=DEV)
        d = buf[guard:guard + B * Cn]
        rc = L.ssl4gie_soft_cross_entropy(x.data_ptr(), 0, t.data_ptr(), 0.9, 0.1 / Cn, loss.data_ptr(), d.data_ptr(),
                                          B, Cn, ws.data_ptr(), torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        assert rc == 0 and bool(torch.isnan(loss))
        d = d.view(B, Cn)
        assert bool(torch.isnan(d[4]).all()) and bool(torch.isfinite(d[[0, 1, 2, 3, 5, 6, 7, 8]]).all())
        assert float(buf[:guard].min()) == 7.0 == float(buf[:guard].max())
        assert float(buf[-guard:].min()) == 7.0 == float(buf[-guard:].max())
    # neither or both of soft_target / label: refused
    assert L.ssl4gie_soft_cross_entropy(x.data_ptr(), 0, 0, 0.9, 0.0, loss.data_ptr(), 0, B, Cn, ws.data_ptr(), 0) == 1000


def test_soft_losses_torch_fallbacks(monkeypatch):
    from ssl4gie_amd.losses import LabelSmoothingCrossEntropy, SoftTargetCrossEntropy
    x, t, y = _loss_case(5, 6, "plain")
    monkeypatch.setenv("SSL4GIE_FUSED_LOSS", "0")
    xd = x.to(DEV).requires_grad_(True)
    for loss in (SoftTargetCrossEntropy()(xd, t.to(DEV)), LabelSmoothingCrossEntropy(0.1)(xd, y.to(DEV))):
        assert not type(loss.grad_fn).__name__.startswith("_SoftCeFn")
    monkeypatch.delenv("SSL4GIE_FUSED_LOSS")
    x3 = x.view(5, 2, 3).to(DEV).requires_grad_(True)   # another rank: the torch formulation
    loss = SoftTargetCrossEntropy()(x3, t.view(5, 2, 3).to(DEV))
    assert not type(loss.grad_fn).__name__.startswith("_SoftCeFn")


# ---------------------------------------------------------------------------------------------- end to end
def test_finetune_step_end_to_end_fp32():
    from ssl4gie_amd.data import Mixup
    from ssl4gie_amd.losses import SoftTargetCrossEntropy
    from ssl4gie_amd.Models.mae.util import lr_sched
    from ssl4gie_amd.Models.mae.util.lr_decay import param_groups_lrd
    from ssl4gie_amd.optim import ArenaAdamW
    g = G(77)
    B, Cn, depth = 6, 10, 3
    m = _small_vit(0.2, seed=9)
    with torch.no_grad():
        m.head.weight.copy_(torch.randn(m.head.weight.shape, generator=g) * 0.2)   # logits of order one
    sd = {k: v.detach().clone().double().requires_grad_(True) for k, v in m.state_dict().items()}
    imgs = torch.randn(B, 3, 64, 64, generator=g)
    y = torch.randint(0, Cn, (B,), generator=g)
    lam, box, use = _mix_tables(B, 64, 64, 0)
    k1, k2 = 1.0 / (1.0 - 0.1), 1.0 / (1.0 - 0.2)
    scales = torch.tensor([[[1, 1, 1, 1, 1, 1], [1, 1, 1, 1, 1, 1]],
                           [[k1, 0, k1, k1, 0, k1], [k1, k1, 0, k1, 0, k1]],
                           [[k2, k2, k2, 0, 0, k2], [0, k2, k2, k2, 0, k2]]], dtype=torch.float32)
    # fp64 restatement
    xm = fc.mixup_images(imgs.double(), lam, box, use)
    tm = fc.mixup_targets(y, lam, Cn, 0.1)
    logits_r = fc.vit_logits(sd, xm, depth, 3, 16, True, drop_scales=scales.double())
    loss_r = fc.soft_target_ce(logits_r, tm)
    loss_r.backward()
    # the engine
    m.to(DEV).set_precision("fp32").train()
    mix = Mixup(mixup_alpha=0.8, cutmix_alpha=1.0, mode="elem", label_smoothing=0.1, num_classes=Cn)
    xd, td = mix.apply_tables(imgs.to(DEV), y.to(DEV), lam.to(DEV), box.to(DEV), use.to(DEV))
    logits = m(xd, drop_scales=scales.to(DEV))
    loss = SoftTargetCrossEntropy()(logits, td)
    loss.backward()
    torch.cuda.synchronize()
    assert logits.dtype == torch.float32 and tuple(logits.shape) == (B, Cn)
    e_logits, e_loss = rel_err(logits.detach(), logits_r.detach()), _scalar_err(loss.detach(), loss_r.detach())
    worst = max((rel_err(p.grad, sd[n].grad), n) for n, p in m.named_parameters())
    print(f"end to end fp32: logits {e_logits:.2e} loss {e_loss:.2e} worst gradient {worst[0]:.2e} ({worst[1]})")
    assert e_logits < 1e-3 and e_loss < 1e-3
    for n, p in m.named_parameters():
        assert p.grad is not None and rel_err(p.grad, sd[n].grad) < 1e-3, n
    # one AdamW step over the layer-decay groups
    groups = param_groups_lrd(m, 0.05, no_weight_decay_list=m.no_weight_decay(), layer_decay=0.75)
    assert len(groups) == 2 * (depth + 2)
    opt = ArenaAdamW(m, groups, lr=1e-3, betas=(0.9, 0.95))
    lr_sched.adjust_learning_rate(opt, 10, argparse.Namespace(lr=1e-3, min_lr=1e-6, warmup_epochs=5, epochs=50))
    before = {n: (p.detach().clone().cpu(), p.grad.detach().clone().cpu()) for n, p in m.named_parameters()}
    hyper = {id(p): (gr["lr"], gr["weight_decay"]) for gr in opt.param_groups for p in gr["params"]}
    assert len({round(h[0], 12) for h in hyper.values()}) == depth + 2
    opt.step()
    torch.cuda.synchronize()
    for n, p in m.named_parameters():
        lr, wd = hyper[id(p)]
        want = fc.adamw_first_step(before[n][0], before[n][1], lr, wd, betas=(0.9, 0.95))
        assert rel_err(p.detach(), want) < 1e-5, n
        assert not torch.equal(p.detach().cpu(), before[n][0]), n
