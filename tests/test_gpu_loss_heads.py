"""GPU parity of the fused loss heads (csrc/loss_ops.hip): MoCo-v3 InfoNCE, the classification finetune's weighted
cross-entropy and the Barlow Twins loss terms.

Every yardstick is the torch formulation in fp64 on the CPU, written out below.  Every bar is
max(1e-5, 8 * e32): e32 is the error of torch's own fp32 formulation on the CPU against the same fp64 result on
the same inputs (1e-5 is the project's bar for this fp32 class, tests/test_gpu_moco.py; the factor 8 allows for a
different summation order and nothing more).  The operands of the Barlow Twins backward are compared bit for bit."""
import functools
from types import SimpleNamespace

import pytest
import torch
import torch.nn.functional as F

from conftest import load_golden, rel_err

pytestmark = pytest.mark.gpu
DEV = "cuda"
EARG = 1000  # SSL4GIE_EARG


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from ssl4gie_amd import _lib
    _lib.load()


def _scalar_err(a, b):
    a = float(a.detach()) if torch.is_tensor(a) else float(a)
    b = float(b)
    return abs(a - b) / (abs(b) if b != 0 else 1.0)


def _bar(e32):
    return max(1e-5, 8.0 * e32)


# ---------------------------------------------------------------------------------------------- InfoNCE
def _nce_torch(q, k, T, off, dtype):
    """builder.py:63-73 on gathered keys, value and dq"""
    q = q.detach().clone().to(dtype).requires_grad_(True)
    qn, kn = F.normalize(q, dim=1), F.normalize(k.to(dtype), dim=1)
    logits = qn @ kn.t() / T
    labels = torch.arange(q.shape[0]) + off
    loss = F.cross_entropy(logits, labels) * (2 * T)
    loss.backward()
    return loss.detach(), q.grad


NCE_CASES = [(5, 7, 24, 2, 1.0), (17, 51, 257, 17, 0.2), (33, 99, 30, 66, 1.0), (48, 96, 256, 48, 0.2),
             (130, 520, 1024, 390, 0.2), (256, 2048, 256, 1792, 1.0), (64, 128, 16, 64, 0.002)]


@functools.lru_cache(maxsize=None)
def _nce_case(idx):
    N, M, C, off, T = NCE_CASES[idx]
    g = torch.Generator("cpu").manual_seed(100 + idx)
    q, k = torch.randn(N, C, generator=g), torch.randn(M, C, generator=g)
    if idx % 2 == 0:
        k[off:off + N] += 0.5 * q          # positives that look like their queries
    k[0] = 0                               # a key of norm 0 (never a positive here: off > 0)
    while True:
        l64, d64 = _nce_torch(q, k, T, off, torch.float64)
        l32, d32 = _nce_torch(q, k, T, off, torch.float32)
        if bool(torch.isfinite(l32)) and bool(torch.isfinite(d32).all()):
            break
        T *= 2                             # only if torch's own fp32 formulation is not finite
    return q, k, T, off, l64, d64, _bar(_scalar_err(l32, l64)), _bar(rel_err(d32, d64))


def _nce_raw(q, k, T, off, want_dq=True, dims=None, fill=None):
    """the entry point itself on device copies; returns rc, loss, dq (buffers pre-filled with `fill`)"""
    from ssl4gie_amd import _lib
    L = _lib.load()
    qd, kd = q.to(DEV).contiguous(), k.to(DEV).contiguous()
    N, M, C = dims or (q.shape[0], k.shape[0], q.shape[1])
    nb = max(L.ssl4gie_infonce_workspace_bytes(q.shape[0], k.shape[0], q.shape[1]), 16)
    ws = torch.zeros(nb, dtype=torch.uint8, device=DEV)
    loss = torch.full((), float("nan") if fill is None else fill, device=DEV)
    dq = torch.full_like(qd, float("nan") if fill is None else fill)
    rc = L.ssl4gie_infonce_loss(qd.data_ptr(), kd.data_ptr(), loss.data_ptr(), dq.data_ptr() if want_dq else 0,
                                N, M, C, float(T), int(off), ws.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return rc, loss.cpu(), dq.cpu(), ws.cpu()


def test_infonce_matches_reference_fixture():
    """G8: the reference's own MoCo.contrastive_loss, value and dq"""
    from ssl4gie_amd.losses import info_nce
    g = load_golden("g8_moco.npz")
    q = torch.from_numpy(g["cl/q"]).to(DEV).requires_grad_(True)
    k = torch.from_numpy(g["cl/k"]).to(DEV)
    assert tuple(q.shape) == (12, 32) and tuple(k.shape) == (12, 32)
    loss = info_nce(q, k, float(g["cl/T"]), 0)
    loss.backward()
    print("g8 loss", float(loss.detach()), float(g["cl/loss"]), "dq err", rel_err(q.grad, g["cl/dq"]))
    assert _scalar_err(loss, g["cl/loss"]) < 1e-5
    assert rel_err(q.grad, g["cl/dq"]) < 1e-4


@pytest.mark.parametrize("idx", range(len(NCE_CASES)))
def test_infonce_value_and_dq_vs_fp64(idx):
    from ssl4gie_amd.losses import info_nce
    q, k, T, off, l64, d64, bar_l, bar_d = _nce_case(idx)
    qd = q.to(DEV).requires_grad_(True)
    loss = info_nce(qd, k.to(DEV), T, off)
    loss.backward()
    el, ed = _scalar_err(loss, l64), rel_err(qd.grad, d64)
    print(f"infonce {NCE_CASES[idx]} T={T}: loss err {el:.2e} (bar {bar_l:.2e}), dq err {ed:.2e} (bar {bar_d:.2e})")
    assert bool(torch.isfinite(loss)) and bool(torch.isfinite(qd.grad).all())
    assert el < bar_l
    assert ed < bar_d


@pytest.mark.parametrize("idx", [1, 5])
def test_infonce_is_deterministic_and_loss_needs_no_gradient(idx):
    q, k, T, off = _nce_case(idx)[:4]
    rc1, l1, d1, _ = _nce_raw(q, k, T, off)
    rc2, l2, d2, _ = _nce_raw(q, k, T, off)
    rc3, l3, d3, _ = _nce_raw(q, k, T, off, want_dq=False)
    assert rc1 == rc2 == rc3 == 0
    assert torch.equal(l1, l2) and torch.equal(d1, d2)
    assert torch.equal(l1, l3) and bool(torch.isnan(d3).all())  # dq = NULL: same loss bits, dq untouched


def test_infonce_backward_scales_with_the_upstream_gradient():
    from ssl4gie_amd.losses import info_nce
    q, k, T, off = _nce_case(2)[:4]
    grads = []
    for factor in (1.0, 3.0):
        qd = q.to(DEV).requires_grad_(True)
        (info_nce(qd, k.to(DEV), T, off) * factor).backward()
        grads.append(qd.grad.cpu())
    assert torch.equal(grads[1], grads[0] * 3.0)


def test_infonce_refuses_what_the_header_refuses():
    q, k = torch.randn(8, 16), torch.randn(24, 16)
    big = torch.randn(2, 1025)
    bad = [("N < 1", q, k, (0, 24, 16), 1.0, 0), ("M < 1", q, k, (8, 0, 16), 1.0, 0), ("C < 1", q, k, (8, 24, 0), 1.0, 0),
           ("C > 1024", big, big, (2, 2, 1025), 1.0, 0), ("T = 0", q, k, None, 0.0, 0), ("T < 0", q, k, None, -1.0, 0),
           ("offset < 0", q, k, None, 1.0, -1), ("offset + N > M", q, k, None, 1.0, 17)]
    for what, a, b, dims, T, off in bad:
        rc, loss, dq, ws = _nce_raw(a, b, T, off, dims=dims, fill=7.0)
        assert rc == EARG, (what, rc)
        assert float(loss) == 7.0 and bool((dq == 7.0).all()) and not bool(ws.any()), what
    assert _nce_raw(q, k, 1.0, 16)[0] == 0  # offset + N == M is the last rank's call


# ---------------------------------------------------------------------------------------------- cross-entropy
CE_CASES = [(1, 2, 1), (7, 6, 1), (256, 12, 1), (130, 1000, 1), (64, 12, 30), (4096, 6, 5), (5, 1, 1)]


@functools.lru_cache(maxsize=None)
def _ce_case(idx, weighted):
    B, C, scale = CE_CASES[idx]
    g = torch.Generator("cpu").manual_seed(200 + idx)
    x = torch.randn(B, C, generator=g) * scale
    t = torch.randint(0, C, (B,), generator=g)
    w = None
    if weighted:
        w = torch.rand(C, generator=g) + 0.1
        if C > 1:
            w[(int(t[0]) + 1) % C] = 0     # one class weight 0 (not the only class present)
    return x, t, w


def _ce_torch(x, t, w, dtype):
    x = x.detach().clone().to(dtype).requires_grad_(True)
    loss = F.cross_entropy(x, t, weight=None if w is None else w.to(dtype))
    loss.backward()
    return loss.detach(), x.grad


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("idx", range(len(CE_CASES)))
def test_cross_entropy_value_and_dlogits_vs_fp64(idx, weighted):
    from ssl4gie_amd.losses import CrossEntropyLoss
    x, t, w = _ce_case(idx, weighted)
    l64, d64 = _ce_torch(x, t, w, torch.float64)
    l32, d32 = _ce_torch(x, t, w, torch.float32)
    bar_l, bar_d = _bar(_scalar_err(l32, l64)), _bar(rel_err(d32, d64))
    fn = CrossEntropyLoss(w).to(DEV)
    runs = []
    for _ in range(2):
        xd = x.to(DEV).requires_grad_(True)
        loss = fn(xd, t.to(DEV))
        loss.backward()
        runs.append((loss.detach().cpu(), xd.grad.cpu()))
    el, ed = _scalar_err(runs[0][0], l64), rel_err(runs[0][1], d64)
    print(f"ce {CE_CASES[idx]} weighted={weighted}: loss err {el:.2e} (bar {bar_l:.2e}), "
          f"dlogits err {ed:.2e} (bar {bar_d:.2e})")
    assert el < bar_l
    assert ed < bar_d
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])  # run to run


@pytest.mark.parametrize("idx", [1, 2, 4])
def test_cross_entropy_bf16_logits(idx):
    """bf16 logits are read as the fp32 values they hold: the loss against fp64 on the same rounded values within the
    bar; the gradient is the fp32 kernel's (held to fp64 above), rounded once to the logits' dtype by autograd"""
    from ssl4gie_amd.losses import CrossEntropyLoss
    x, t, w = _ce_case(idx, True)
    xb = x.to(torch.bfloat16)
    l64, d64 = _ce_torch(xb.float(), t, w, torch.float64)
    l32, d32 = _ce_torch(xb.float(), t, w, torch.float32)
    fn = CrossEntropyLoss(w).to(DEV)
    xd = xb.to(DEV).requires_grad_(True)
    loss = fn(xd, t.to(DEV))
    loss.backward()
    xf = xb.float().to(DEV).requires_grad_(True)
    loss_f = fn(xf, t.to(DEV))
    loss_f.backward()
    assert loss.dtype == torch.float32 and xd.grad.dtype == torch.bfloat16
    assert _scalar_err(loss, l64) < _bar(_scalar_err(l32, l64))
    assert rel_err(xf.grad, d64) < _bar(rel_err(d32, d64))
    assert torch.equal(loss, loss_f) and torch.equal(xd.grad, xf.grad.to(torch.bfloat16))


def test_cross_entropy_torch_fallbacks(monkeypatch):
    """SSL4GIE_FUSED_LOSS=0 and inputs of another rank run the torch formulation"""
    from ssl4gie_amd.losses import CrossEntropyLoss
    x, t, w = _ce_case(2, True)
    fn = CrossEntropyLoss(w).to(DEV)
    monkeypatch.setenv("SSL4GIE_FUSED_LOSS", "0")
    assert torch.equal(fn(x.to(DEV), t.to(DEV)), F.cross_entropy(x.to(DEV), t.to(DEV), weight=w.to(DEV)))
    monkeypatch.delenv("SSL4GIE_FUSED_LOSS")
    x4 = x[:, :, None, None].expand(-1, -1, 2, 2).contiguous().to(DEV)
    t4 = t[:, None, None].expand(-1, 2, 2).contiguous().to(DEV)
    # torch's own reduction over a map of targets is not bit-stable from call to call on the device
    a, b = float(fn(x4, t4)), float(F.cross_entropy(x4, t4, weight=w.to(DEV)))
    assert abs(a - b) <= 1e-6 * abs(b)


def test_cross_entropy_target_out_of_range_is_nan_and_stays_in_bounds():
    from ssl4gie_amd import _lib
    L = _lib.load()
    B, C, guard = 9, 6, 64
    g = torch.Generator("cpu").manual_seed(5)
    x = torch.randn(B, C, generator=g).to(DEV)
    t = torch.randint(0, C, (B,), generator=g)
    t[4] = C                                # one past the last class
    t = t.to(DEV)
    w = (torch.rand(C, generator=g) + 0.1).to(DEV)
    buf = torch.full((guard + B * C + guard,), float("nan"), device=DEV)
    before = buf.view(torch.int32).clone()
    loss = torch.zeros((), device=DEV)
    ws = torch.zeros(L.ssl4gie_cross_entropy_workspace_bytes(B, C), dtype=torch.uint8, device=DEV)
    d = buf[guard:guard + B * C]
    rc = L.ssl4gie_cross_entropy(x.data_ptr(), t.data_ptr(), w.data_ptr(), loss.data_ptr(), d.data_ptr(), B, C,
                                 ws.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert rc == 0
    assert bool(torch.isnan(loss))
    after = buf.view(torch.int32)
    assert torch.equal(after[:guard], before[:guard]) and torch.equal(after[-guard:], before[-guard:])
    d = d.view(B, C).cpu()
    assert bool(torch.isnan(d[4]).all())
    assert bool(torch.isfinite(torch.cat([d[:4], d[5:]])).all())


# ---------------------------------------------------------------------------------------------- Barlow Twins terms
LAMBD = 0.0051
BT_DIMS = [1, 200, 256, 1000, 129]   # 129: odd and several tiles, the element-wise path of the operand kernel
BT_SCALES = [1.0 / 512, 3.0 / 1024, 1.0, 1.0 / 512, 3.0 / 1024]
# the operand check also beyond 1024 (the width of the projector the method is used with): odd, and a multiple of 4
BT_GRAD_DIMS = BT_DIMS + [1025, 1028]
BT_GRAD_SCALES = BT_SCALES + [1.0 / 512, 3.0 / 1024]


@functools.lru_cache(maxsize=None)
def _bt_c(D):
    g = torch.Generator("cpu").manual_seed(300 + D)
    return 0.05 * torch.randn(D, D, generator=g) + 0.9 * torch.eye(D)


@pytest.mark.parametrize("D", BT_DIMS)
def test_bt_loss_vs_fp64(D):
    from ssl4gie_amd import ops
    from ssl4gie_amd.Models.barlow_twins import cross_corr_loss_terms
    c = _bt_c(D)
    c64 = c.double()
    d64 = torch.diagonal(c64)
    l64 = (d64 - 1).pow(2).sum() + LAMBD * (c64.pow(2).sum() - d64.pow(2).sum())
    l32, _ = cross_corr_loss_terms(c.clone(), LAMBD)
    bar = _bar(_scalar_err(l32, l64))
    cd = c.to(DEV)
    a, b = ops.bt_loss(cd, LAMBD), ops.bt_loss(cd, LAMBD)
    err = _scalar_err(a, l64)
    print(f"bt loss D={D}: err {err:.2e} (bar {bar:.2e})")
    assert err < bar
    assert torch.equal(a, b)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("D,scale", list(zip(BT_GRAD_DIMS, BT_GRAD_SCALES)))
def test_bt_grad_operands_equal_the_torch_ops_bit_for_bit(D, scale, dtype):
    from ssl4gie_amd import ops
    from ssl4gie_amd.Models.barlow_twins import cross_corr_loss_terms
    c = _bt_c(D)
    s = torch.tensor(scale, dtype=torch.float32)
    _, dc = cross_corr_loss_terms(c.clone(), LAMBD)   # c * (2 lambda), diagonal 2 (c - 1)
    want = (dc * s).to(dtype)                          # dc * (g / n_global), then the operand cast
    w, wt = ops.bt_loss_grad(c.to(DEV), s.to(DEV), dtype, LAMBD)
    assert w.dtype == dtype and wt.dtype == dtype
    assert torch.equal(w.cpu(), want)
    assert torch.equal(wt.cpu(), want.t().contiguous())
    assert torch.equal(wt.t(), w)


# ---------------------------------------------------------------------------------------------- wiring
def test_moco_contrastive_loss_switch(monkeypatch):
    from ssl4gie_amd.Models.moco_v3.moco.builder import MoCo
    q, k, T, off, l64, d64, bar_l, bar_d = _nce_case(3)
    q, k = q[:, :], k[off:off + q.shape[0]]            # one process: keys of this rank only, labels arange(n)
    _, d64 = _nce_torch(q, k, T, 0, torch.float64)
    _, d32 = _nce_torch(q, k, T, 0, torch.float32)
    res = {}
    for sw in ("0", "1"):
        monkeypatch.setenv("SSL4GIE_FUSED_INFONCE", sw)
        qd = q.to(DEV).requires_grad_(True)
        loss = MoCo.contrastive_loss(SimpleNamespace(T=T), qd, k.to(DEV))
        loss.backward()
        res[sw] = (float(loss.detach()), qd.grad.cpu())
    assert abs(res["1"][0] - res["0"][0]) < 1e-5 * abs(res["0"][0])
    assert rel_err(res["1"][1], res["0"][1]) < _bar(rel_err(d32, d64))
    assert not torch.equal(res["1"][1], res["0"][1])   # two different code paths did run


def test_moco_resnet_step_with_the_fused_loss(monkeypatch):
    from functools import partial
    from ssl4gie_amd.Models.moco_v3.moco import builder
    from ssl4gie_amd.Models.resnet import resnet50
    g = torch.Generator("cpu").manual_seed(11)
    x1 = torch.randn(8, 3, 64, 64, generator=g).to(DEV)
    x2 = torch.randn(8, 3, 64, 64, generator=g).to(DEV)
    losses = {}
    for sw in ("0", "1"):
        monkeypatch.setenv("SSL4GIE_FUSED_INFONCE", sw)
        torch.manual_seed(0)
        m = builder.MoCo_ResNet(partial(resnet50, zero_init_residual=True), 256, 4096, 0.2)
        m.to(DEV).set_precision("fp32")
        loss = m(x1, x2, 0.99)
        loss.backward()
        torch.cuda.synchronize()
        losses[sw] = float(loss.detach())
        grads = [p.grad for p in m.parameters() if p.requires_grad]
        assert len(grads) > 50 and all(gr is not None and bool(torch.isfinite(gr).all()) for gr in grads)
    assert abs(losses["1"] - losses["0"]) < 1e-5 * abs(losses["0"])


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_barlow_twins_head_step_with_the_fused_loss_terms(prec, monkeypatch):
    from ssl4gie_amd.engine import EngineModule
    from ssl4gie_amd.Models.barlow_twins import BarlowTwins

    class Feat(EngineModule):
        def forward_cls(self, x):
            return x

    g = torch.Generator("cpu").manual_seed(1)
    a = torch.randn(48, 64, generator=g)
    b = a + 0.5 * torch.randn(48, 64, generator=g)
    res = {}
    for sw in ("0", "1"):
        monkeypatch.setenv("SSL4GIE_FUSED_BT_LOSS", sw)
        torch.manual_seed(0)
        m = BarlowTwins(Feat(), 64, "128-264", lambd=LAMBD).to(DEV).set_precision(prec)
        x1, x2 = a.to(DEV).requires_grad_(True), b.to(DEV).requires_grad_(True)
        loss = m(x1, x2)
        loss.backward()
        torch.cuda.synchronize()
        grads = [p.grad for p in m.parameters() if p.requires_grad]
        assert grads and all(gr is not None and bool(torch.isfinite(gr).all()) for gr in grads)
        res[sw] = (float(loss.detach()), x1.grad.cpu(), x2.grad.cpu())
    assert abs(res["1"][0] - res["0"][0]) < 1e-5 * abs(res["0"][0])
    # the operands of the two backward GEMMs are bit-identical by construction, so is everything after them
    assert torch.equal(res["1"][1], res["0"][1]) and torch.equal(res["1"][2], res["0"][2])
