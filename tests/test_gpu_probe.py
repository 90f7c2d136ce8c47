"""GPU parity of the linear-probe device code (csrc/probe_ops.hip, the SGD step of csrc/optim_ops.hip and what drives
them): ssl4gie_topk_update and ssl4gie_sgd_arena against the restatements of tests/probe_checks.py, the ranged optimizers, the BatchNorm head on the
reference's recorded run (G22), the frozen-trunk step end to end, and the unchanged Linear-head path.

Bars: counts and ranks exact; losses max(1e-5, 8 * e32) with e32 the error of torch's own fp32 formulation on the CPU
against fp64 on the same inputs (the rule of tests/test_gpu_loss_heads.py), measured per row as |a - b| / max(1, |b|);
optimizer updates 1e-5 (tests/test_gpu_optim.py); model quantities in fp32 1e-3, the project's fp32 bar; bf16 per tensor
within 1.5 x the reference's own bf16-autocast error stored in the fixture."""
import copy
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import finetune_checks as fc
import probe_checks as pc
from conftest import load_golden, rel_err

pytestmark = pytest.mark.gpu
DEV = "cuda"
NAN = float("nan")


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


def _row_err(a, b):
    """max over the rows of |a - b| / max(1, |b|); NaNs must sit in the same rows"""
    a, b = a.double().cpu(), b.double().cpu()
    assert torch.equal(a.isnan(), b.isnan())
    keep = ~b.isnan()
    if not bool(keep.any()):
        return 0.0
    return float(((a[keep] - b[keep]).abs() / b[keep].abs().clamp(min=1.0)).max())


# ---------------------------------------------------------------------------------------------- topk_update
@functools.lru_cache(maxsize=None)
def _topk_case(B, C, dtype, nans=False):
    """logits as the kernel sees them (rounded to `dtype`), targets, and the restatement on those numbers.  Rows, as far
    as B reaches: 0 target 0 | 1 an all-equal row | 2 target -1 | 3 target C | 4 logits +-1e4, target on -1e4 | 5 1e4 on
    the target | 6 target C - 1 | 7 the target's value repeated at a lower and a higher column | nans: 8 a NaN beside
    the target, 9 a NaN on the target, 10 both"""
    g = G(1000 * B + C + (7 if dtype == torch.bfloat16 else 0))
    x = 3.0 * torch.randn(B, C, generator=g)
    t = torch.randint(0, C, (B,), generator=g)
    t[0] = 0
    if B > 1:
        x[1] = 0.75
        t[1] = min(2, C - 1)
    if B > 2:
        t[2] = -1
    if B > 10:
        t[3] = C
        x[4, 0], x[4, 1], t[4] = 1e4, -1e4, 1
        x[5, 3], t[5] = 1e4, 3
        t[6] = C - 1
        x[7, 0] = x[7, C - 1] = x[7, 2]
        t[7] = 2
        if nans:
            x[8, 1], t[8] = NAN, 0
            x[9, 4], t[9] = NAN, 4
            x[10, 0], x[10, 4], t[10] = NAN, NAN, 4
    x = x.to(dtype).float()   # everything below is scored on the rounded numbers: ties are covered by the rule, not avoided
    rank = pc.ranks(x, t)
    loss64 = pc.row_losses(x, t)
    ok = (t >= 0) & (t < C)
    loss32 = torch.where(ok, F.cross_entropy(x, t.clamp(0, C - 1), reduction="none"), torch.zeros(B))
    return x, t, rank, loss64, _bar(_row_err(loss32, loss64))


def _ks(C):
    return sorted({1, 2, 5, C})


def _guarded(n, dtype, fill):
    """a buffer of n elements with 16 poisoned elements on either side: (whole, the n in the middle)"""
    whole = torch.full((n + 32,), fill, dtype=dtype, device=DEV)
    return whole, whole[16:16 + n]


def _run_topk(x, t, ks, ld, dtype, with_rows=True):
    """the entry point on device copies laid out with row stride ld inside guard bands; every buffer is checked for
    writes outside its own elements"""
    from ssl4gie_amd import ops
    B, C = x.shape
    lw, flat = _guarded(B * ld, dtype, 7.0)
    logits = flat.view(B, ld)[:, :C]
    logits.copy_(x.to(dtype))
    aw, acc = _guarded(len(ks) + 2, torch.int64, -77)
    sw, loss_sum = _guarded(1, torch.float64, -5.5)
    rw, rank = _guarded(B, torch.int32, -99)
    ow, row_loss = _guarded(B, torch.float32, -9.25)
    acc.zero_()
    loss_sum.zero_()
    ww, ws = _guarded(int(ops.topk_workspace(B, DEV).numel()), torch.uint8, 0xAB)
    before = [w.clone() for w in (lw, aw, sw, rw, ow, ww)]
    ops.topk_update(acc, loss_sum, logits, t.to(DEV), ks, rank if with_rows else None,
                    row_loss if with_rows else None, workspace=ws)
    torch.cuda.synchronize()
    assert torch.equal(lw.view(torch.int16 if dtype == torch.bfloat16 else torch.int32),
                       before[0].view(torch.int16 if dtype == torch.bfloat16 else torch.int32)), "logits were written"
    for w, b0, n in ((aw, before[1], len(ks) + 2), (sw, before[2], 1), (rw, before[3], B), (ow, before[4], B),
                     (ww, before[5], ws.numel())):
        assert torch.equal(w[:16], b0[:16]) and torch.equal(w[16 + n:], b0[16 + n:]), "a guard band was written"
    if not with_rows:
        assert torch.equal(rw, before[3]) and torch.equal(ow.view(torch.int32), before[4].view(torch.int32))
    return acc.cpu(), loss_sum.cpu(), rank.cpu(), row_loss.cpu()


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("C", [5, 63, 64, 65, 1000, 1003])
@pytest.mark.parametrize("B", [1, 3, 257])
def test_topk_update_vs_restatement(B, C, dtype):
    x, t, rank_r, loss_r, bar = _topk_case(B, C, dtype)
    ks = _ks(C)
    want = pc.topk_counts(rank_r, ks)
    rows = {}
    for ld in (C, C + 3):
        acc, loss_sum, rank, row_loss = _run_topk(x, t, ks, ld, dtype)
        assert acc.tolist() == want, (ld, acc.tolist(), want)
        assert torch.equal(rank.long(), rank_r), ld
        e_rows = _row_err(row_loss, loss_r)
        e_sum = abs(float(loss_sum) - float(loss_r.sum())) / max(1.0, abs(float(loss_r.sum())))
        print(f"topk B={B} C={C} ld={ld} {dtype}: row loss err {e_rows:.2e} sum err {e_sum:.2e} bar {bar:.2e}")
        assert e_rows < bar and e_sum < bar
        # the fixed order: rows in index order over 256 threads, then a tree, in fp64 — bit for bit
        assert float(loss_sum) == pc.tree_sum_rows(row_loss.tolist())
        rows[ld] = row_loss
    assert torch.equal(rows[C].view(torch.int32), rows[C + 3].view(torch.int32)), "a row's loss depends on its alignment"
    if B > 1:   # the all-equal row: a hit at k iff target < k
        assert int(rank_r[1]) == min(2, C - 1)
    if B > 10:
        assert torch.isfinite(loss_r[4]) and float(loss_r[4]) > 1.9e4 and float(row_loss[5]) == 0.0
        assert rank[2] == -1 and rank[3] == -1 and float(row_loss[2]) == 0.0 and float(row_loss[3]) == 0.0
        assert int(rank_r[7]) >= 1   # the equal value at column 0 is ordered above the target's


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("C", [63, 1003])
def test_topk_update_nan_rows(C, dtype):
    """a NaN orders above every number (NaNs among themselves by index), the row's loss is NaN and reaches loss_sum;
    without the optional per-row outputs nothing but the accumulators and the workspace is written"""
    x, t, rank_r, loss_r, bar = _topk_case(257, C, dtype, True)
    ks = _ks(C)
    acc, loss_sum, rank, row_loss = _run_topk(x, t, ks, C + 3, dtype)
    assert acc.tolist() == pc.topk_counts(rank_r, ks) and torch.equal(rank.long(), rank_r)
    assert row_loss[8:11].isnan().all() and _row_err(row_loss, loss_r) < bar
    assert bool(loss_sum.isnan())
    assert int(rank_r[9]) == 0 and int(rank_r[10]) == 1 and int(rank_r[8]) >= 1
    acc2, loss_sum2, _, _ = _run_topk(x, t, ks, C, dtype, with_rows=False)
    assert torch.equal(acc2, acc) and bool(loss_sum2.isnan())


def test_topk_updates_add_up_and_repeat_bit_for_bit():
    from ssl4gie_amd import ops
    x, t, rank_r, loss_r, bar = _topk_case(257, 1003, torch.float32)
    ks = [1, 5]
    xd, td = x.to(DEV), t.to(DEV)
    runs = []
    for _ in range(2):
        acc = torch.zeros(4, dtype=torch.int64, device=DEV)
        loss_sum = torch.zeros(1, dtype=torch.float64, device=DEV)
        parts, want = [], 0.0
        for lo, hi in ((0, 100), (100, 201), (201, 257)):
            row_loss = torch.empty(hi - lo, device=DEV)
            ops.topk_update(acc, loss_sum, xd[lo:hi], td[lo:hi], ks, row_loss=row_loss)
            want += pc.tree_sum_rows(row_loss.tolist())   # ((0 + s1) + s2) + s3
            parts.append(pc.topk_counts(rank_r[lo:hi], ks))
        assert acc.tolist() == [sum(p[i] for p in parts) for i in range(4)] == pc.topk_counts(rank_r, ks)
        assert float(loss_sum) == want
        runs.append(loss_sum.cpu())
    assert torch.equal(runs[0].view(torch.int64), runs[1].view(torch.int64))


def test_topk_update_refuses_bad_arguments():
    from ssl4gie_amd import _lib, ops
    L = _lib.load()
    x = torch.zeros(4, 8, device=DEV)
    t = torch.zeros(4, dtype=torch.int64, device=DEV)
    acc = torch.zeros(4, dtype=torch.int64, device=DEV)
    s = torch.zeros(1, dtype=torch.float64, device=DEV)
    ws = ops.topk_workspace(4, DEV)
    import ctypes

    def call(ks, ld=8, C=8):
        arr = (ctypes.c_int * len(ks))(*ks)
        return L.ssl4gie_topk_update(x.data_ptr(), _lib.F32, ld, t.data_ptr(), arr, len(ks), acc.data_ptr(), s.data_ptr(),
                                     0, 0, 4, C, ws.data_ptr(), 0)
    assert call([1, 5]) == 0
    for bad in ([0, 5], [1, 9], [5, 1], [2, 2], list(range(1, 10)), []):
        assert call(bad) == 1000, bad
    assert call([1], ld=7) == 1000
    assert L.ssl4gie_topk_workspace_bytes(0) == 0 and L.ssl4gie_topk_workspace_bytes(257) >= 4 * 257
    with pytest.raises(ValueError):
        ops.topk_update(acc, s, x, t, [1, 9])
    torch.cuda.synchronize()


def test_topk_accuracy_and_accuracy_on_the_device(monkeypatch):
    """the class and the drivers' function on device tensors equal their torch formulation (SSL4GIE_FUSED_METRICS=0)
    and the restatement: bf16 logits, a strided view, three batches, one read-back"""
    from ssl4gie_amd.metrics import TopKAccuracy, accuracy
    x, t, rank_r, loss_r, bar = _topk_case(257, 1000, torch.bfloat16)
    wide = torch.zeros(257, 1024, dtype=torch.bfloat16, device=DEV)
    wide[:, :1000] = x.to(DEV)
    xd, td = wide[:, :1000], t.to(DEV)
    res = {}
    for flag in ("1", "0"):
        monkeypatch.setenv("SSL4GIE_FUSED_METRICS", flag)
        m = TopKAccuracy((1, 5))
        for lo, hi in ((0, 100), (100, 201), (201, 257)):
            m.update(xd[lo:hi], td[lo:hi])
        res[flag] = m.compute()
        a = accuracy(xd, td, topk=(1, 5))
        assert all(v.is_cuda and tuple(v.shape) == (1,) for v in a)
        res["a" + flag] = [float(v) for v in a]
    want = pc.topk_counts(rank_r, (1, 5))
    for flag in ("1", "0"):
        r = res[flag]
        assert (r["n"], r["rejected"]) == (want[2], want[3])
        assert r["acc1"] == 100.0 * want[0] / want[2] and r["acc5"] == 100.0 * want[1] / want[2]
        assert abs(r["loss"] - float(loss_r.sum()) / want[2]) < bar * max(1.0, abs(float(loss_r.sum()) / want[2]))
    assert res["a1"] == res["a0"]
    assert all(abs(a - 100.0 * w / 257) < 1e-4 for a, w in zip(res["a1"], want))
    with pytest.raises(ValueError):
        TopKAccuracy((1, 5)).update(xd[:, :4], td)


# ---------------------------------------------------------------------------------------------- crop rule on the device
@pytest.mark.parametrize("Hs,Ws", pc.CROP_SIZES)
def test_tf_rrc_boxes_on_the_device_equals_the_python_loop(Hs, Ws):
    """the same uniforms as tests/test_probe_cpu.py, which shows that no pre-rounding side is within 5e-5 of a
    half-integer: a 1-ulp difference of the device's fp32 exp cannot flip a rounding"""
    from ssl4gie_amd.data import tf_rrc_boxes
    u = pc.crop_uniforms()
    want, _ = pc.tf_boxes(u, Hs, Ws)
    got = tf_rrc_boxes(u.to(DEV), Hs, Ws)
    assert got.is_cuda and got.dtype == torch.int32 and torch.equal(got.cpu(), want)


def test_mae_linprobe_transform_runs_the_crop_kernel():
    from ssl4gie_amd import ops
    from ssl4gie_amd.data import DeviceImageBank, MAELinprobeTransform
    g = G(31)
    imgs = torch.randint(0, 256, (6, 40, 56, 3), generator=g, dtype=torch.uint8)
    bank = DeviceImageBank.from_uint8(imgs, DEV)
    idx = torch.tensor([5, 0, 3, 3], device=DEV)
    t = MAELinprobeTransform(32, generator=torch.Generator(DEV).manual_seed(4))
    out = t(bank, idx)
    gen = torch.Generator(DEV).manual_seed(4)
    box, flip = MAELinprobeTransform(32, generator=gen).draw(4, 40, 56, DEV)
    want = ops.view_sample_u8(bank.images, idx, box, flip, 32, "bicubic", t.mean, t.std)
    assert tuple(out.shape) == (4, 3, 32, 32) and torch.equal(out, want)


# ---------------------------------------------------------------------------------------------- sgd_arena
SEGS = (64, 192, 128)


def _poisoned(n, seed):
    """fp32 [64 + n + 64] of NaNs with distinct payloads: any write shows"""
    g = G(seed)
    bits = torch.randint(0, 1 << 20, (n + 128,), generator=g, dtype=torch.int32) | 0x7FC00000
    return bits.view(torch.float32).clone()


@pytest.mark.parametrize("momentum,wd", [(0.0, 0.0), (0.9, 0.0), (0.0, 1e-2), (0.9, 1e-2)])
def test_sgd_arena_vs_fp64(momentum, wd):
    from ssl4gie_amd import _lib
    L = _lib.load()
    n = sum(SEGS)
    g = G(5)
    p, buf = _poisoned(n, 1), _poisoned(n, 2)
    active = torch.ones(n, dtype=torch.bool)
    active[64:256] = False                         # the middle segment is skipped
    live = torch.zeros(n + 128, dtype=torch.bool)
    live[64:64 + n] = active
    p[live] = torch.randn(int(active.sum()), generator=g)
    buf[live] = 0.0
    pd, bd = p.to(DEV), buf.to(DEV)
    start = torch.tensor([0, 64, 256, 384], dtype=torch.int64, device=DEV)
    lr = torch.tensor([0.1, -1.0, 0.05], device=DEV)
    wds = torch.tensor([wd, 123.0, wd], device=DEV)
    lr_el = torch.cat([torch.full((64,), 0.1), torch.zeros(192), torch.full((128,), 0.05)]).double()
    p64, b64 = p[64:64 + n].double(), buf[64:64 + n].double()
    for step in range(3):
        gr = _poisoned(n, 10 + step)
        gr[live] = torch.randn(int(active.sum()), generator=g)
        gd = gr.to(DEV)
        rc = L.ssl4gie_sgd_arena(pd.data_ptr() + 256, gd.data_ptr() + 256, bd.data_ptr() + 256, start.data_ptr(),
                                 lr.data_ptr(), wds.data_ptr(), 3, momentum, n, 0)
        assert rc == 0
        pn, bn = pc.sgd_step(p64, gr[64:64 + n].double(), b64, lr_el, momentum, wd)
        p64, b64 = torch.where(active, pn, p64), torch.where(active, bn, b64)
    torch.cuda.synchronize()
    po, bo = pd.cpu(), bd.cpu()
    assert rel_err(po[live], p64[active]) < 1e-5 and rel_err(bo[live], b64[active]) < 1e-5
    assert not torch.equal(po[live], p[live])
    # the skipped segment, its buffer and everything outside the n elements: bit-unchanged
    assert torch.equal(po.view(torch.int32)[~live], p.view(torch.int32)[~live])
    assert torch.equal(bo.view(torch.int32)[~live], buf.view(torch.int32)[~live])
    assert L.ssl4gie_sgd_arena(pd.data_ptr() + 256, gd.data_ptr() + 256, bd.data_ptr() + 256, start.data_ptr(),
                               lr.data_ptr(), wds.data_ptr(), 3, momentum, n + 2, 0) == 1000
    assert L.ssl4gie_sgd_arena(pd.data_ptr() + 260, gd.data_ptr() + 256, bd.data_ptr() + 256, start.data_ptr(),
                               lr.data_ptr(), wds.data_ptr(), 3, momentum, n, 0) == 1000


def _toy():
    from ssl4gie_amd.engine import EngineModule

    class Toy(EngineModule):
        def __init__(self):
            super().__init__()
            self.a = torch.nn.Linear(40, 72)
            self.b = torch.nn.Linear(72, 24)
            self.norm = torch.nn.LayerNorm(24)
            self.c = torch.nn.Linear(24, 10)
    torch.manual_seed(0)
    return Toy().to(DEV)


def _fake_grads(m, seed):
    g = G(seed)
    for _, p in m.named_parameters():
        p.grad = torch.randn(p.shape, generator=g).to(DEV)


def _outside(a, lo, hi, own):
    """the arena's bits outside [lo, hi) plus those of every segment inside it that is not one of `own`"""
    keep = torch.ones(a.numel, dtype=torch.bool)
    ends = list(a.offsets[1:]) + [a.numel]
    for p, o, e in zip(a.params, a.offsets, ends):
        if any(p is q for q in own):
            keep[o:e] = False
    return a.data.detach().cpu().view(torch.int32)[keep]


@pytest.mark.parametrize("momentum,wd", [(0.0, 0.0), (0.9, 1e-2)])
def test_arena_sgd_steps_only_its_hull(momentum, wd):
    """own = (a.bias, b.bias): the hull also covers b.weight, which has a gradient and must not move"""
    from ssl4gie_amd.optim import ArenaSGD
    m = _toy()
    a = m.arena()
    own = [m.a.bias, m.b.bias]
    ref = [torch.nn.Parameter(p.detach().clone()) for p in own]
    topt = torch.optim.SGD(ref, lr=0.1, momentum=momentum, weight_decay=wd)
    opt = ArenaSGD(m, own, lr=0.1, momentum=momentum, weight_decay=wd)
    lo, hi = a.span([m.a.bias, m.b.weight, m.b.bias])
    before = _outside(a, lo, hi, own)
    for step in range(3):
        _fake_grads(m, 20 + step)
        for r, p in zip(ref, own):
            r.grad = p.grad.detach().clone()
        if step == 2:
            for gr in opt.param_groups + topt.param_groups:
                gr["lr"] = 0.03
        opt.step()
        topt.step()
    torch.cuda.synchronize()
    for r, p in zip(ref, own):
        assert rel_err(p.detach(), r.detach()) < 1e-5
    assert opt.buf.numel() == hi - lo < a.numel
    assert torch.equal(_outside(a, lo, hi, own), before)
    sd = opt.state_dict()
    assert sd["kind"] == "ArenaSGD" and sd["state"]["buf"].numel() == hi - lo and sd["step_count"] == 3
    opt2 = ArenaSGD(m, own, lr=0.5, momentum=momentum, weight_decay=wd)
    opt2.load_state_dict(sd)
    assert opt2.param_groups[0]["lr"] == 0.03 and torch.equal(opt2.buf.cpu(), opt.buf.cpu())
    opt2.buf = torch.zeros(8)
    with pytest.raises(ValueError):
        opt2.step()


def test_ranged_lars_equals_arena_lars_and_keeps_to_its_hull():
    from ssl4gie_amd.Models.mae.util.lars import LARS
    from ssl4gie_amd.optim import ArenaLARS
    m1 = _toy()
    m2 = copy.deepcopy(m1)
    a1, a2 = m1.arena(), m2.arena()
    own1, own2 = [m1.b.weight, m1.b.bias], [m2.b.weight, m2.b.bias]
    opt1 = LARS(iter(own1), lr=0.8, weight_decay=1e-3)
    opt2 = ArenaLARS(m2, own2, lr=0.8, weight_decay=1e-3)
    lo, hi = a1.span(own1)
    before = _outside(a1, lo, hi, own1)
    start = [p.detach().clone() for p in own1]
    for step in range(3):
        _fake_grads(m1, 40 + step)
        for p, q in zip(m1.parameters(), m2.parameters()):
            q.grad = p.grad.detach().clone()
        if step == 1:
            opt1.param_groups[0]["lr"] = opt2.param_groups[0]["lr"] = 0.4   # lr_sched.adjust_learning_rate
        opt1.step()
        opt2.step()
    torch.cuda.synchronize()
    for p, q, p0 in zip(own1, own2, start):
        assert rel_err(p.detach(), q.detach()) < 1e-6 and not torch.equal(p.detach(), p0)
    assert opt1.mu.numel() == hi - lo and opt2.mu.numel() == a2.numel and hi - lo < a1.numel
    assert rel_err(opt1.mu, opt2.mu[lo:hi]) < 1e-6
    assert torch.equal(_outside(a1, lo, hi, own1), before)
    # fp64 restatement of the reference's rule, from the same start
    p64 = [p.double().cpu() for p in start]
    mu64 = [torch.zeros_like(p) for p in p64]
    for step in range(3):
        grads = {}
        g = G(40 + step)
        for n, p in m1.named_parameters():
            grads[n] = torch.randn(p.shape, generator=g).double()
        lr = 0.8 if step == 0 else 0.4
        for i, n in enumerate(("b.weight", "b.bias")):
            p64[i], mu64[i] = pc.lars_step(p64[i], grads[n], mu64[i], lr, 1e-3, 0.9, 0.001)
    for p, r in zip(own1, p64):
        assert rel_err(p.detach(), r) < 1e-5


# ---------------------------------------------------------------------------------------------- G22: the BatchNorm head
NAMES = ("loss", "weight", "bias", "running_mean", "running_var")


def _g22_run(prec):
    from ssl4gie_amd.losses import CrossEntropyLoss
    from ssl4gie_amd.Models.mae.models_vit import VisionTransformer
    from ssl4gie_amd.Models.mae.util.lars import LARS
    from ssl4gie_amd.probe import mae_linear_probe
    g = load_golden("g22_linprobe.npz")
    torch.manual_seed(1)
    m = mae_linear_probe(VisionTransformer(img_size=32, embed_dim=192, depth=1, num_heads=3, num_classes=10))
    with torch.no_grad():
        m.head[1].weight.copy_(torch.from_numpy(g["weight0"]))
        m.head[1].bias.copy_(torch.from_numpy(g["bias0"]))
    m.to(DEV).set_precision(prec).train()
    opt = LARS(m.head.parameters(), lr=float(g["lr"]), weight_decay=float(g["weight_decay"]),
               momentum=float(g["momentum"]), trust_coefficient=float(g["trust_coefficient"]))
    crit = CrossEntropyLoss()
    x, t = torch.from_numpy(g["x"]).to(DEV), torch.from_numpy(g["target"]).to(DEV)
    out = {k: [] for k in NAMES}
    for s in range(x.shape[0]):
        logits = m.forward_head(x[s])
        assert logits.dtype == torch.float32
        loss = crit(logits, t[s])
        opt.zero_grad()
        loss.backward()
        opt.step()
        out["loss"].append(loss.detach().double().cpu().reshape(1))
        out["weight"].append(m.head[1].weight.detach().double().cpu())
        out["bias"].append(m.head[1].bias.detach().double().cpu())
        out["running_mean"].append(m.head[0].running_mean.detach().double().cpu())
        out["running_var"].append(m.head[0].running_var.detach().double().cpu())
    sd = m.state_dict()
    assert int(sd["head.0.num_batches_tracked"]) == x.shape[0]
    assert all(p.grad is None for n, p in m.named_parameters() if not n.startswith("head."))
    return g, {k: torch.stack(v) for k, v in out.items()}


def test_g22_probe_head_fp32():
    """every stored quantity of every step of the reference's own run (its LARS, torch's BatchNorm1d / Linear /
    CrossEntropyLoss, fp32) within 1e-3"""
    g, out = _g22_run("fp32")
    for k in NAMES:
        for s in range(out[k].shape[0]):
            e = rel_err(out[k][s].reshape(g[f"fp32/{k}"][s].shape), g[f"fp32/{k}"][s])
            print(f"g22 fp32 step {s} {k}: {e:.2e}")
            assert e < 1e-3, (k, s, e)


def test_g22_probe_head_bf16():
    """relative L2 error against the reference's fp64 run within 1.5 x the error of the reference's own bf16-autocast
    run (tests/golden/make_golden_linprobe.py), the G17 rule (tests/test_gpu_models_golden.py::_bf16_gate): weight,
    bias and both running statistics per tensor at EVERY step; the loss, one number per step, as the tensor it is
    recorded as — the 5-step curve — at 1.5 x, and each step at 3 x the reference's worst step, G17's clause for tiny
    tensors ("a single draw of a heavy-tailed quantity in either arithmetic").  Measured on the MI355X, engine
    (reference autocast) per step: loss 3.5e-5 (1.0e-5), 8.0e-5 (1.1e-4), 1.4e-4 (1.1e-4), 2.7e-4 (4.4e-5), 6.7e-5
    (3.3e-4) — step by step a single loss is above 1.5 x twice and below 0.25 x once; weight 1.3e-5 .. 8.6e-5
    (1.7e-5 .. 1.1e-4); bias 1.0e-3 .. 2.0e-3 (2.1e-3 .. 6.9e-3); running statistics at fp32 rounding level in both."""
    g, out = _g22_run("bf16")
    worst = []
    errs = {}
    for k in NAMES:
        for s in range(out[k].shape[0]):
            ref = torch.from_numpy(g[f"fp64/{k}"][s]).double().reshape(out[k][s].shape)
            e = float((out[k][s] - ref).norm() / ref.norm())
            errs[k, s] = e
            bar = 1.5 * float(g[f"bf16_err/{k}"][s])
            print(f"g22 bf16 step {s} {k}: {e:.3e} (reference autocast {float(g[f'bf16_err/{k}'][s]):.3e})")
            if k != "loss" and e > bar:
                worst.append((k, s, e, bar))
    l64 = torch.from_numpy(g["fp64/loss"]).double().flatten()
    curve = float((out["loss"].flatten() - l64).norm() / l64.norm())
    ref_curve = float((torch.from_numpy(g["bf16_err/loss"]).double() * l64).norm() / l64.norm())
    print(f"g22 bf16 loss curve: {curve:.3e} (reference autocast {ref_curve:.3e})")
    assert not worst, worst
    assert curve <= 1.5 * ref_curve, (curve, ref_curve)
    assert max(errs["loss", s] for s in range(l64.numel())) <= 3.0 * float(g["bf16_err/loss"].max())


# ---------------------------------------------------------------------------------------------- end to end
def _probe_vit(seed=9):
    from ssl4gie_amd.Models.mae.models_vit import VisionTransformer
    torch.manual_seed(seed)
    m = VisionTransformer(img_size=64, embed_dim=192, depth=3, num_heads=3, num_classes=10)
    g = G(seed)
    with torch.no_grad():   # biases and affine tables away from their zero / one initialisation
        for n, p in m.named_parameters():
            if p.ndim == 1:
                p.add_(0.1 * torch.randn(p.shape, generator=g))
    return m


def test_linear_probe_end_to_end_fp32():
    from ssl4gie_amd.losses import CrossEntropyLoss
    from ssl4gie_amd.Models.mae.util.lars import LARS
    from ssl4gie_amd.probe import mae_linear_probe, sanity_check
    B, steps, lr = 8, 3, 6.4   # the recipe's rate: LARS moves the weight by 0.64 % of its norm per step
    m = mae_linear_probe(_probe_vit())
    g = G(11)
    imgs = torch.randn(steps, B, 3, 64, 64, generator=g)
    y = torch.randint(0, 10, (steps, B), generator=g)
    sd = {k: v.detach().clone().double() for k, v in m.state_dict().items()}
    pretrained = {"module.base_encoder." + k: v.detach().clone() for k, v in m.state_dict().items()}
    # fp64 restatement: the trunk of tests/finetune_checks.py with an identity head gives the features
    eye = {**sd, "head.weight": torch.eye(192, dtype=torch.float64), "head.bias": torch.zeros(192, dtype=torch.float64)}
    feats = torch.stack([fc.vit_logits(eye, imgs[s].double(), 3, 3, 16, False) for s in range(steps)])
    curve = pc.probe_head_curve(feats, y, sd["head.1.weight"], sd["head.1.bias"], lr, 0.0, 0.9, 0.001)
    # the engine
    m.to(DEV).set_precision("fp32").train()
    opt = LARS(m.head.parameters(), lr=lr, weight_decay=0.0)
    crit = CrossEntropyLoss()
    x0 = imgs[0].to(DEV)
    f_train = m.forward_features(x0)
    with torch.no_grad():
        f_nograd = m.forward_features(x0)
    assert not f_train.requires_grad and torch.equal(f_train, f_nograd), "the frozen forward is the no_grad forward"
    assert rel_err(f_train, feats[0]) < 1e-3
    trunk0 = {k: v.detach().clone() for k, v in m.state_dict().items() if not k.startswith("head.")}
    for s in range(steps):
        logits = m(imgs[s].to(DEV))
        loss = crit(logits, y[s].to(DEV))
        opt.zero_grad()
        loss.backward()
        opt.step()
        loss_r, w_r, b_r, rm_r, rv_r, logits_r = curve[s]
        errs = (rel_err(logits.detach(), logits_r), abs(float(loss.detach()) - float(loss_r)) / abs(float(loss_r)),
                rel_err(m.head[1].weight.detach(), w_r), rel_err(m.head[1].bias.detach(), b_r),
                rel_err(m.head[0].running_mean, rm_r), rel_err(m.head[0].running_var, rv_r))
        print(f"probe end to end step {s}: logits {errs[0]:.2e} loss {errs[1]:.2e} weight {errs[2]:.2e} bias "
              f"{errs[3]:.2e} running mean {errs[4]:.2e} var {errs[5]:.2e}")
        assert max(errs) < 1e-3, (s, errs)
    torch.cuda.synchronize()
    assert not torch.equal(m.head[1].weight.detach().cpu().double(), sd["head.1.weight"])
    now = m.state_dict()
    for k, v in trunk0.items():
        assert torch.equal(now[k], v), k            # every trunk parameter and buffer bit-unchanged
    for n, p in m.named_parameters():
        assert (p.grad is None) == (not n.startswith("head.")), n
    sanity_check({k: v for k, v in now.items() if not k.startswith("head.")}, pretrained, "head")
    with pytest.raises(AssertionError, match="head.0.running_mean is changed"):
        sanity_check(now, pretrained, "head.1")     # the BatchNorm head's statistics did move
    # eval(): the running statistics
    m.eval()
    logits = m(imgs[0].to(DEV))
    _, w_r, b_r, rm_r, rv_r, _ = curve[-1]
    assert rel_err(logits, pc.bn_head_eval(feats[0], w_r, b_r, rm_r, rv_r)) < 1e-3


def test_resnet50_fc_probe_step_eval_mode_fp32():
    """the 'fc' arm of main_lincls.py: eval() trunk (BatchNorm on its running statistics), fc alone trains.  No
    eval-mode BatchNorm backward is reached (it would raise), no running statistic moves, fc's gradients are the fp64
    product of the engine's own pooled features, and one ArenaSGD step is torch.optim.SGD's"""
    from ssl4gie_amd.losses import CrossEntropyLoss
    from ssl4gie_amd.Models.resnet import resnet50
    from ssl4gie_amd.optim import ArenaSGD
    from ssl4gie_amd.probe import moco_linear_probe
    torch.manual_seed(3)
    m = moco_linear_probe(resnet50(num_classes=10), "fc")
    g = G(13)
    with torch.no_grad():
        for mod in m.modules():
            if isinstance(mod, torch.nn.BatchNorm2d):   # a pre-trained trunk's statistics are not 0 / 1
                mod.running_mean.copy_(0.1 * torch.randn(mod.running_mean.shape, generator=g))
                mod.running_var.copy_(0.5 + torch.rand(mod.running_var.shape, generator=g))
    m.to(DEV).set_precision("fp32").eval()
    imgs = torch.randn(4, 3, 64, 64, generator=g).to(DEV)
    y = torch.randint(0, 10, (4,), generator=g)
    before = {k: v.detach().clone() for k, v in m.state_dict().items()}
    with torch.no_grad():
        pooled = m.pooled(imgs).double().cpu()
    logits = m(imgs)
    assert logits.dtype == torch.float32 and tuple(logits.shape) == (4, 10)
    loss = CrossEntropyLoss()(logits, y.to(DEV))
    loss.backward()
    w64, b64 = before["fc.weight"].double().cpu(), before["fc.bias"].double().cpu()
    logits_r = pooled @ w64.t() + b64
    loss_r, gw, gb = pc.ce_head_grads(logits_r, y, pooled)
    assert rel_err(logits.detach(), logits_r) < 1e-3 and abs(float(loss.detach()) - float(loss_r)) < 1e-3 * abs(float(loss_r))
    assert rel_err(m.fc.weight.grad, gw) < 1e-3 and rel_err(m.fc.bias.grad, gb) < 1e-3
    assert all(p.grad is None for n, p in m.named_parameters() if not n.startswith("fc."))
    opt = ArenaSGD(m, [p for p in m.parameters() if p.requires_grad], 0.1, momentum=0.9, weight_decay=1e-4)
    gw32, gb32 = m.fc.weight.grad.detach().double().cpu(), m.fc.bias.grad.detach().double().cpu()
    opt.step()
    torch.cuda.synchronize()
    w1, _ = pc.sgd_step(w64, gw32, torch.zeros_like(w64), 0.1, 0.9, 1e-4)
    b1, _ = pc.sgd_step(b64, gb32, torch.zeros_like(b64), 0.1, 0.9, 1e-4)
    assert rel_err(m.fc.weight.detach(), w1) < 1e-5 and rel_err(m.fc.bias.detach(), b1) < 1e-5
    assert opt.buf.numel() == 2048 * 10 + 64
    now = m.state_dict()
    for k, v in before.items():
        if not k.startswith("fc."):
            assert torch.equal(now[k], v), k        # running statistics included
    assert not torch.equal(now["fc.weight"], before["fc.weight"])


# ---------------------------------------------------------------------------------------------- unchanged path
@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_plain_linear_head_is_the_parent_call_sequence(prec):
    """VisionTransformer with an nn.Linear head: logits and gradients bit-equal to `_linear(forward_features(x), head)`
    called directly, which is what forward() was before the head forms were added"""
    m = _probe_vit(seed=4).to(DEV).set_precision(prec).train()
    g = G(17)
    x = torch.randn(4, 3, 64, 64, generator=g).to(DEV)
    w = torch.randn(4, 10, generator=g).to(DEV)
    res = []
    for which in ("forward", "direct", "forward_head"):
        for p in m.parameters():
            p.grad = None
        if which == "forward":
            logits = m(x)
        elif which == "direct":
            logits = m._linear(m.forward_features(x), m.head, out_dtype=torch.float32)
        else:
            logits = m.forward_head(m.forward_features(x))
        (logits * w).sum().backward()
        torch.cuda.synchronize()
        res.append((logits.detach().clone(), {n: p.grad.detach().clone() for n, p in m.named_parameters()}))
    for logits, grads in res[1:]:
        assert torch.equal(res[0][0], logits)
        for n, gr in grads.items():
            assert torch.equal(res[0][1][n], gr), n
