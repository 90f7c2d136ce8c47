"""GPU: backward through fixed BatchNorm statistics — ssl4gie_bn_bwd_frozen per element against fp64, BatchNormFn in
evaluation mode and under FrozenBatchNorm2d against fp64 autograd, and the ResNet50 trunk with
norm_layer=FrozenBatchNorm2d against the torchvision restatement with its BatchNorms in eval().

Kernel reference: `bn_checks.ref_backward(dy, mask, x, mean, rstd, gamma, inv_count=1, sums=zeros)` — with zero sums
the training-mode expression IS the frozen one (dx = rstd gamma g; tests/test_frozen_bn_cpu.py pins it to autograd
through F.batch_norm(training=False)) and the mag of its bound is |a| |g|, so the bounds, rho and K are those of
bn_checks, unchanged.  The masks: MASK_Y and MASK_BITS read what they are handed (y > 0 of a stored output / its bit
map), so they have no ties; MASK_X re-decides the signs from x, and an element whose fp64 pre-activation lies inside
bn_checks' tie radius is undecidable — its dy is set to 0 on both sides (at most MAX_TIE_SHARE of a case).
The fixed statistics of a case are the fp32 batch statistics of its x (bn_checks.fp32_eval), so `edge_case`'s choice
of seeds keeps the ties under that cap here too.  rows = 1 runs without ReLU, as in the training-mode module; the
exact-integer family covers the masks there."""
import math

import pytest
import torch
import torch.nn.functional as F

import bn_checks as bc
from conftest import rel_err
from test_frozen_bn_cpu import check_frozen_argument_validation
from test_gpu_batchnorm_kernels import exact_inputs, pack_bits, unpack_bits

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32, BF, F64 = torch.float32, torch.bfloat16, torch.float64
NONE, Y, XM, BITS = range(4)            # SSL4GIE_BN_MASK_*
KIND = {NONE: "none", Y: "y", XM: "x", BITS: "bits"}


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from ssl4gie_amd import _lib
    _lib.load()


def dn(dtype):
    return "bf16" if dtype == BF else "fp32"


def G(seed):
    return torch.Generator("cpu").manual_seed(seed)


# ===================================================================== the kernel, real-valued
def frozen_inputs(c):
    """case -> (mean, rstd: the fp32 batch statistics of x, taken as the fixed ones; y: the stored output the masks
    are read from; per mask kind (mask tensor for the kernel, boolean reference mask, dy))"""
    o = bc.fp32_eval(c)
    mean, rstd, y, dy = o["mean"].contiguous(), o["rstd"].contiguous(), o["y"], c["dy"]
    forms = {NONE: (None, None, dy)}
    if c["relu"]:
        forms[Y] = (y, y > 0, dy)
        if c["dtype"] == BF:
            forms[BITS] = (pack_bits(y > 0), y > 0, dy)
        pre, mag = bc.ref_forward(c["x"], mean, rstd, c["gamma"], c["beta"], None)
        tie = pre.abs() < bc.K["y"] * bc.EPS32 * mag
        share = float(tie.sum()) / tie.numel()
        assert share <= bc.MAX_TIE_SHARE, "%.3g of the elements are ReLU ties (cap %g)" % (share, bc.MAX_TIE_SHARE)
        forms[XM] = (None, pre > 0, torch.where(tie, torch.zeros_like(dy), dy))
    return mean, rstd, forms


def run_frozen(rep, c, tag, targets=("none", "both")):
    """every legal mask kind x {with, without dres} x `targets` x accumulate of one case through check_backward"""
    from ssl4gie_amd import ops
    x, gamma, beta, dt, C = c["x"], c["gamma"], c["beta"], c["dtype"], c["C"]
    mean, rstd, forms = frozen_inputs(c)
    zeros = torch.zeros(2, C, dtype=F64, device=DEV)
    for kind, (mask, ref_mask, dy) in forms.items():
        bw = bc.ref_backward(dy, ref_mask, x, mean, rstd, gamma, 1.0, zeros)
        for want_dres in ((True,) if kind == BITS else (False,) if kind == XM else (False, True)):
            first = None
            for tg in targets:
                for acc in (False, True):
                    dg = db = dg0 = db0 = None
                    if tg in ("both", "dgamma"):
                        dg0 = c["dg0"] if acc else None
                        dg = c["dg0"].clone() if acc else torch.full_like(c["dg0"], math.nan)
                    if tg in ("both", "dbeta"):
                        db0 = c["db0"] if acc else None
                        db = c["db0"].clone() if acc else torch.full_like(c["db0"], math.nan)
                    reads_x = kind == XM or dg is not None
                    dx, dres = ops.bn_bwd_frozen(dy, kind, mask, x if reads_x else None, gamma,
                                                 beta if kind == XM else None, mean if reads_x else None, rstd,
                                                 want_dres, dg, db, acc)
                    assert (dres is not None) == want_dres
                    t = "%smask=%s dres=%d grads=%s acc=%d." % (tag, KIND[kind], want_dres, tg, acc)
                    bc.check_backward(rep, bw, dt, dx, dres, None, dg, db, dg0, db0, tag=t)
                    if first is None:
                        first = dx
                    elif not torch.equal(dx, first):      # one dx whatever else the call writes
                        rep.fail(t + "dx", "differs from the dx of the form without parameter gradients")


def finish(rep):
    worst = {}
    for k, v in rep.worst.items():      # error / (2^-24 mag), the worst per kind of output
        worst[k.rsplit(".", 1)[-1]] = max(worst.get(k.rsplit(".", 1)[-1], 0.0), v)
    print({k: round(v, 3) for k, v in sorted(worst.items())})
    rep.assert_ok()


C_BF = (8, 24, 64, 72, 512, 2048)


@pytest.mark.parametrize("C,dtype", [(C, BF) for C in C_BF] + [(C, F32) for C in (4, 12) + C_BF],
                         ids=lambda v: dn(v) if isinstance(v, torch.dtype) else "C%d" % v)
def test_frozen_backward_real_row_edges(C, dtype):
    """rows 1, 2, 3 and the lane-step edges; gamma = 0, gamma < 0 and a constant channel are in every case (make_case);
    gamma NULL and the single-target forms (dbeta alone passes no x) at the last row count"""
    rep = bc.Report()
    rows_list = bc.edge_rows(C, dtype)
    for rows in rows_list:
        if C < 8:     # make_case places its special channels up to index 5
            c = small_case(rows, C, dtype, rows > 1)
        else:
            c = bc.to_device(bc.edge_case(rows, C, dtype, rows > 1, False, True), DEV)
        run_frozen(rep, c, "rows %d: " % rows)
    if C >= 8:
        c = bc.to_device(plain_relu_case(rows_list[-1], C, dtype, False), DEV)
        run_frozen(rep, c, "no affine: ")
        c = bc.to_device(bc.edge_case(rows_list[-2], C, dtype, True, False, True), DEV)
        run_frozen(rep, c, "single target: ", targets=("dbeta", "dgamma"))
    finish(rep)


def plain_relu_case(rows, C, dtype, with_res):
    """edge_case for BatchNorm WITHOUT affine parameters in front of a ReLU: make_case's constant channel has the
    pre-activation (x - mean) rstd = 0 there, a tie in every row, so it is given values like the others'; the seed is
    chosen as edge_case chooses it"""
    for s in range(64):
        c = bc.make_case(rows, C, dtype, "cpu", bc.edge_seed(rows, C) + 1000003 * s, True, with_res, False)
        c["x"][:, 3] = (0.75 * c["x"][:, 6].float() + 0.5).to(dtype)
        o = bc.fp32_eval(c)
        rep = bc.Report({n: 2 * v for n, v in bc.K.items()})
        bc.check_forward(rep, c["x"], o["mean"], o["rstd"], None, None, c["res"], True, o["y"])
        if rep.worst["tie_share"] <= bc.MAX_TIE_SHARE:
            return c
    raise AssertionError("no seed keeps the ReLU ties of %d x %d within the cap" % (rows, C))


def small_case(rows, C, dtype, relu):
    """C = 4 (fp32): the channels of an 8-wide case that carry make_case's specials 1 .. 4 (gamma = beta = 0,
    gamma = 0, the constant channel, gamma < 0)"""
    c = bc.edge_case(rows, 8, dtype, relu, False, True)
    cut = lambda v: v[..., 1:1 + C].contiguous() if torch.is_tensor(v) else v
    c = {k: cut(v) for k, v in c.items()}
    c["C"] = C
    return bc.to_device(c, DEV)


@pytest.mark.parametrize("dtype", [F32, BF], ids=dn)
def test_frozen_backward_real_33_partitions(dtype):
    """the parameter-gradient form over 33 partitions (and the flat form at a size of several blocks)"""
    rows, C, parts = bc.PARTITION_SHAPES[3]
    assert parts == 33 == bc.bn_parts(rows, C)
    rep = bc.Report()
    c = bc.make_case(rows, C, dtype, DEV, 4242, True, False, True)
    run_frozen(rep, c, "")
    finish(rep)


# ===================================================================== the kernel, exact integers
@pytest.mark.parametrize("dtype", [F32, BF], ids=dn)
@pytest.mark.parametrize("C", [8, 72])
def test_frozen_backward_exact_every_row_count_1_to_300(C, dtype):
    """small-integer dy and x, integer mean, power-of-two rstd and gamma: every product and every partial sum is exact
    in fp32 (and dx = a g, |a g| <= 24, in bf16), so dx, dres, dbeta and dgamma equal the integer results bit for bit —
    one map, every prefix of its rows, from the flat form and from the reduction form (accumulating on odd counts)"""
    from ssl4gie_amd import ops
    R = 300
    e = exact_inputs(R, C, dtype, 7 * C + 1)
    x, dy, y, mean, rstd, gamma, beta = e["x"], e["dy"], e["y"], e["mean"], e["rstd"], e["gamma"], e["beta"]
    gamma = torch.where(gamma == 3.0, torch.full_like(gamma, 4.0), gamma)     # powers of two (and 0, negatives)
    a = rstd.to(F64) * gamma.to(F64)
    masks = {NONE: (None, None), Y: (y, y > 0),
             XM: (None, x.to(F64) * a + (beta.to(F64) - mean.to(F64) * a) > 0)}
    if dtype == BF:
        masks[BITS] = (e["bits"], unpack_bits(e["bits"], R, C))       # a prefix of the rows is a prefix of the bytes
    xhat = (x.to(F64) - mean.to(F64)) * rstd.to(F64)
    ok = {}
    for kind, (mask, ref_mask) in masks.items():
        g = dy.to(F64) if ref_mask is None else torch.where(ref_mask, dy.to(F64), torch.zeros((), dtype=F64, device=DEV))
        assert 2 * float((g * xhat).abs().sum(0).max()) < 2 ** 24 and float((g * a).abs().max()) <= 32
        dx_ref, s1, s2 = g * a, g.cumsum(0), (g * xhat).cumsum(0)
        want_dres = kind != XM
        o = ok[kind] = torch.ones(R, 6, dtype=torch.bool, device=DEV)
        for rows in range(1, R + 1):
            m = mask if mask is None else (mask[:rows * C // 8] if kind == BITS else mask[:rows])
            xs = x[:rows]
            dx, dres = ops.bn_bwd_frozen(dy[:rows], kind, m, xs if kind == XM else None, gamma,
                                         beta if kind == XM else None, mean if kind == XM else None, rstd, want_dres,
                                         None, None, False)
            o[rows - 1, 0] = (dx.to(F64) == dx_ref[:rows]).all()
            if want_dres:
                o[rows - 1, 1] = (dres.to(F64) == g[:rows]).all()
            acc = bool(rows & 1)
            dg, db = (e["dg0"].clone(), e["db0"].clone()) if acc else (torch.full_like(e["dg0"], math.nan),
                                                                       torch.full_like(e["db0"], math.nan))
            dx, dres = ops.bn_bwd_frozen(dy[:rows], kind, m, xs, gamma, beta if kind == XM else None, mean, rstd,
                                         want_dres, dg, db, acc)
            o[rows - 1, 2] = (dx.to(F64) == dx_ref[:rows]).all()
            if want_dres:
                o[rows - 1, 3] = (dres.to(F64) == g[:rows]).all()
            o[rows - 1, 4] = (db.to(F64) == s1[rows - 1] + (e["db0"].to(F64) if acc else 0)).all()
            o[rows - 1, 5] = (dg.to(F64) == s2[rows - 1] + (e["dg0"].to(F64) if acc else 0)).all()
    names = ("dx (flat)", "dres (flat)", "dx (reduction)", "dres (reduction)", "dbeta", "dgamma")
    bad = ["mask=%s %s at rows = %s" % (KIND[k], names[j], (~o[:, j]).nonzero().flatten().add(1).tolist()[:20])
           for k, o in ok.items() for j in range(6) if not bool(o[:, j].all())]
    assert not bad, "\n".join(bad)


def test_every_illegal_pointer_combination_is_an_argument_error_and_launches_nothing():
    """host buffers behind every pointer: a launch on them would fault, an argument error returns before it"""
    torch.cuda.synchronize()
    accepted, rejected = check_frozen_argument_validation()
    torch.cuda.synchronize()    # and the device is as it was
    assert accepted == 104 and rejected > 30000


# ===================================================================== BatchNormFn with fixed statistics
def _bn_pair(c, frozen):
    """the holder of case c's fixed statistics: FrozenBatchNorm2d, or nn.BatchNorm2d / BatchNorm1d in eval()"""
    from ssl4gie_amd.Models.resnet import FrozenBatchNorm2d
    C = c["C"]
    o = bc.fp32_eval(c)
    affine = c["gamma"] is not None
    bn = FrozenBatchNorm2d(C, eps=c["eps"]) if frozen else torch.nn.BatchNorm2d(C, eps=c["eps"], affine=affine)
    bn.to(DEV)
    with torch.no_grad():
        bn.running_mean.copy_(o["mean"])
        bn.running_var.copy_(o["var"])
        if affine:
            bn.weight.copy_(c["gamma"])
            bn.bias.copy_(c["beta"])
    return bn.train() if frozen else bn.eval()     # a FrozenBatchNorm2d ignores the flag


def _run_fn(bn, c, dy, relu, with_res):
    from ssl4gie_amd.engine import GradSink
    from ssl4gie_amd.resnet_engine import BatchNormFn
    shp = (2, 5, 7, c["C"])
    x = c["x"].clone().view(shp).requires_grad_(True)
    res = c["res"].clone().view(shp).requires_grad_(True) if with_res else None
    w, b = getattr(bn, "weight", None), getattr(bn, "bias", None)
    y = BatchNormFn.apply(x, w, b, res, bn, relu, GradSink(None))
    saved = [t for t in y.grad_fn.saved_tensors if t is not None]
    y.backward(dy.view(shp))
    gw = w.grad if (w is not None and w.requires_grad) else None
    gb = b.grad if (b is not None and b.requires_grad) else None
    return y.detach(), x, x.grad, res.grad if with_res else None, gw, gb, saved


@pytest.mark.parametrize("dtype", [F32, BF], ids=dn)
@pytest.mark.parametrize("affine", [False, True], ids=["plain", "affine"])
@pytest.mark.parametrize("with_res", [False, True], ids=["nores", "res"])
@pytest.mark.parametrize("relu", [False, True], ids=["id", "relu"])
@pytest.mark.parametrize("C", [8, 64])
def test_batchnorm_fn_backward_through_fixed_statistics(C, relu, with_res, affine, dtype):
    """[2, 5, 7, C] maps through BatchNormFn under eval() (the parent raises NotImplementedError here) and under
    FrozenBatchNorm2d: dx, dres, dgamma and dbeta against fp64 autograd through F.batch_norm(training=False) under
    bn_checks' bounds (ReLU ties carry no gradient on either side); the two holders bit-identical; x not saved"""
    rows = 70
    c = plain_relu_case(rows, C, dtype, with_res) if (relu and not affine) else \
        bc.edge_case(rows, C, dtype, relu, with_res, affine)
    c = bc.to_device(c, DEV)
    bn = _bn_pair(c, False)
    # fp64 autograd from the module's own buffers
    xr = c["x"].to(F64).requires_grad_(True)
    rr = c["res"].to(F64).requires_grad_(True) if with_res else None
    gr = c["gamma"].to(F64).requires_grad_(True) if affine else None
    br = c["beta"].to(F64).requires_grad_(True) if affine else None
    pre = F.batch_norm(xr, bn.running_mean.to(F64), bn.running_var.to(F64), gr, br, False, 0.1, bn.eps)
    if with_res:
        pre = pre + rr
    dy = c["dy"]
    if relu:
        _, mag = bc.ref_forward(c["x"], bn.running_mean, (bn.running_var.to(F64) + bn.eps) ** -0.5, c["gamma"],
                                c["beta"], c["res"])
        tie = pre.detach().abs() < bc.K["y"] * bc.EPS32 * mag
        assert float(tie.sum()) / tie.numel() <= bc.MAX_TIE_SHARE
        dy = torch.where(tie, torch.zeros_like(dy), dy)
    (F.relu(pre) if relu else pre).backward(dy.to(F64))
    rstd64 = (bn.running_var.to(F64) + bn.eps) ** -0.5
    bw = bc.ref_backward(dy, (pre.detach() > 0) if relu else None, c["x"], bn.running_mean, rstd64, c["gamma"], 1.0,
                         torch.zeros(2, C, dtype=F64, device=DEV))
    assert float((bw["dx"] - xr.grad).abs().max()) <= 1e-12 * float(xr.grad.abs().max() + 1e-300)
    bw["dx"] = xr.grad
    if affine:
        bw["s1"], bw["s2"] = br.grad, gr.grad
    rep = bc.Report()
    y, x, dx, dres, dg, db, saved = _run_fn(bn, c, dy, relu, with_res)
    bc.check_backward(rep, bw, dtype, dx.view(rows, C), dres.view(rows, C) if with_res else None, None, dg, db,
                      tag="eval: ")
    assert (dg is not None) == affine and (db is not None) == affine
    if with_res:
        assert rep.failed or torch.equal(dres.view(rows, C).to(F64), rr.grad)
    if not affine:     # nothing wants x: the convolution output is not kept alive
        assert all(t.data_ptr() != x.data_ptr() for t in saved)
    if affine:
        fz = _bn_pair(c, True)
        assert fz.training and not list(fz.parameters())
        y2, x2, dx2, dres2, dg2, db2, saved2 = _run_fn(fz, c, dy, relu, with_res)
        bc.check_backward(rep, bw, dtype, dx2.view(rows, C), dres2.view(rows, C) if with_res else None, tag="frozen: ")
        assert dg2 is None and db2 is None and fz.weight.grad is None and fz.bias.grad is None
        assert torch.equal(y, y2) and torch.equal(dx, dx2), "FrozenBatchNorm2d and eval() BatchNorm2d differ"
        assert not with_res or torch.equal(dres, dres2)
        assert all(t.data_ptr() != x2.data_ptr() for t in saved2), "the frozen forward saved x"
        ptrs = {t.data_ptr() for t in saved2}
        if relu and not (with_res and dtype == BF):
            assert y2.data_ptr() in ptrs, "the ReLU output is the mask"
        elif relu:
            assert any(t.dtype == torch.uint8 and t.numel() == rows * C // 8 for t in saved2), "the bit map is the mask"
            assert y2.data_ptr() not in ptrs
        # the constants are computed once per module and again when a buffer is rewritten
        cache = fz.__dict__["_ssl4gie_frozen"]
        _run_fn(fz, c, dy, relu, with_res)
        assert fz.__dict__["_ssl4gie_frozen"] is cache
        with torch.no_grad():
            fz.running_var.mul_(4.0)
        y3 = _run_fn(fz, c, dy, relu, with_res)[0]
        assert fz.__dict__["_ssl4gie_frozen"] is not cache and not torch.equal(y3, y2)
    finish(rep)


def test_eval_batchnorm1d_and_syncbatchnorm_take_the_same_path():
    """BatchNorm1d over [N, C] and an (unconverted, single-process) SyncBatchNorm in eval(): no exchange, the same
    numbers as BatchNorm2d"""
    from ssl4gie_amd.engine import GradSink
    from ssl4gie_amd.resnet_engine import BatchNormFn, SYNC_BN_COLLECTIVES, SYNC_BN_DIRECT
    C = 64
    c = bc.to_device(bc.edge_case(70, C, F32, True, False, True), DEV)
    ref = _bn_pair(c, False)
    outs = []
    before = (SYNC_BN_COLLECTIVES[0], SYNC_BN_DIRECT[0])
    for cls in (torch.nn.BatchNorm2d, torch.nn.BatchNorm1d, torch.nn.SyncBatchNorm):
        bn = cls(C, eps=c["eps"]).to(DEV)
        bn.load_state_dict(ref.state_dict())
        bn.eval()
        x = c["x"].clone().requires_grad_(True)
        y = BatchNormFn.apply(x, bn.weight, bn.bias, None, bn, True, GradSink(None))
        y.backward(c["dy"])
        outs.append((y.detach(), x.grad, bn.weight.grad, bn.bias.grad))
        assert torch.equal(bn.running_mean, ref.running_mean) and torch.equal(bn.running_var, ref.running_var)
        assert int(bn.num_batches_tracked) == 0
    assert (SYNC_BN_COLLECTIVES[0], SYNC_BN_DIRECT[0]) == before
    for o in outs[1:]:
        assert all(torch.equal(a, b) for a, b in zip(o, outs[0]))


# ===================================================================== ResNet50 with norm_layer=FrozenBatchNorm2d
def nchw(x):
    return x.permute(0, 3, 1, 2).contiguous()


def _l2(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).norm() / (b.norm() + 1e-300))


def _ref_maps(net, imgs):
    x = net.maxpool(net.relu(net.bn1(net.conv1(imgs))))
    maps = []
    for layer in (net.layer1, net.layer2, net.layer3, net.layer4):
        x = layer(x)
        maps.append(x)
    return maps


@pytest.fixture(scope="module")
def trunk():
    """weights with random non-trivial BatchNorm buffers, the input, the loss weights, and the restatement's maps and
    gradients with its BatchNorms in eval(): in fp64 (the reference) and in fp32 under bf16 autocast (its own error)"""
    from oracle import torchvision_restatement as tvr
    from ssl4gie_amd.Models.resnet import FrozenBatchNorm2d, ResNet50
    torch.manual_seed(17)
    m = ResNet50(norm_layer=FrozenBatchNorm2d)
    g = G(18)
    with torch.no_grad():
        for mod in m.modules():
            if isinstance(mod, FrozenBatchNorm2d):
                n = mod.weight.shape
                mod.weight.copy_(0.5 + torch.rand(n, generator=g))
                mod.bias.copy_(0.2 * torch.randn(n, generator=g))
                mod.running_mean.copy_(0.2 * torch.randn(n, generator=g))
                mod.running_var.copy_(0.5 + torch.rand(n, generator=g))
    sd = {k: v.detach().clone() for k, v in m.state_dict().items()}
    imgs = torch.randn(2, 3, 64, 64, generator=g)
    shapes = [(2, 256, 16, 16), (2, 512, 8, 8), (2, 1024, 4, 4), (2, 2048, 2, 2)]
    ws = [torch.randn(s, generator=g) for s in shapes]

    def run(dt, autocast):
        net = tvr.resnet50()
        res = net.load_state_dict(sd, strict=False)
        assert not res.unexpected_keys and all(k.startswith("fc.") or k.endswith("num_batches_tracked")
                                               for k in res.missing_keys)
        net.to(dt).eval()
        with torch.autocast("cpu", dtype=torch.bfloat16, enabled=autocast):
            maps = _ref_maps(net, imgs.to(dt))
        assert [tuple(t.shape) for t in maps] == shapes
        sum((t.to(dt) * w.to(dt)).sum() for t, w in zip(maps, ws)).backward()
        grads = {k: p.grad for k, p in net.named_parameters() if k in sd and "bn" not in k and "downsample.1" not in k}
        return [t.detach() for t in maps], grads
    maps64, g64 = run(F64, False)
    maps_ac, g_ac = run(F32, True)
    own = {"map%d" % (i + 1): _l2(a, b) for i, (a, b) in enumerate(zip(maps_ac, maps64))}
    own.update({k: _l2(g_ac[k], g64[k]) for k in g64})
    return {"sd": sd, "imgs": imgs, "ws": ws, "maps": maps64, "grads": g64, "autocast_err": own}


def _engine_step(trunk, precision, trainable):
    from ssl4gie_amd.Models.resnet import FrozenBatchNorm2d, ResNet50
    from ssl4gie_amd.optim import ArenaAdamW
    m = ResNet50(norm_layer=FrozenBatchNorm2d)
    m.load_state_dict(trunk["sd"], strict=True)
    m.to(DEV).set_precision(precision)
    m.freeze_stages(trainable)
    maps = m.forward_maps(trunk["imgs"].to(DEV), all_stages=True)
    loss = sum((t.float() * w.to(DEV).permute(0, 2, 3, 1)).sum() for t, w in zip(maps, trunk["ws"]))
    loss.backward()
    grads = {k: (p.grad.detach().clone() if p.grad is not None else None) for k, p in m.named_parameters()}
    # one optimizer step: what is frozen stays bit for bit, what trains moves
    before = {k: v.detach().clone() for k, v in m.state_dict().items()}
    ArenaAdamW(m, list(m.parameters()), lr=1e-2).step()
    after = m.state_dict()
    names = dict(m.named_parameters())
    for k, v in before.items():
        moves = k in names and names[k].requires_grad
        assert torch.equal(after[k], v) != moves, (k, "moved" if not moves else "did not move")
    return maps, grads


@pytest.fixture(scope="module")
def steps(trunk):
    return {(p, k): _engine_step(trunk, p, k) for p in ("fp32", "bf16") for k in (5, 3)}


@pytest.mark.parametrize("trainable", [5, 3])
def test_frozen_resnet50_fp32_within_1e3_of_the_fp64_restatement(trunk, steps, trainable):
    maps, grads = steps[("fp32", trainable)]
    errs = {"map%d" % (i + 1): rel_err(nchw(t.detach().float()), r) for i, (t, r) in enumerate(zip(maps, trunk["maps"]))}
    for k, gref in trunk["grads"].items():
        if grads[k] is not None:
            errs[k] = rel_err(grads[k], gref)
    print("worst:", sorted(errs.items(), key=lambda kv: -kv[1])[:5])
    assert len(errs) == 4 + (53 if trainable == 5 else 42)
    assert max(errs.values()) < 1e-3, {k: v for k, v in errs.items() if not v < 1e-3}


@pytest.mark.parametrize("trainable", [5, 3])
def test_frozen_resnet50_bf16_within_1p5x_the_restatements_own_autocast_error(trunk, steps, trainable):
    """per tensor (the four maps and every trainable weight's gradient): relative L2 error against the fp64
    restatement <= 1.5 x the error of the restatement itself under torch.autocast(bfloat16)"""
    maps, grads = steps[("bf16", trainable)]
    errs = {"map%d" % (i + 1): _l2(nchw(t.detach().float()), r) for i, (t, r) in enumerate(zip(maps, trunk["maps"]))}
    for k, gref in trunk["grads"].items():
        if grads[k] is not None:
            errs[k] = _l2(grads[k], gref)
    own = trunk["autocast_err"]
    print("worst ratios:", sorted(((round(errs[k] / own[k], 3), k, errs[k], own[k]) for k in errs), reverse=True)[:5])
    assert len(errs) == 4 + (53 if trainable == 5 else 42)
    bad = {k: (v, own[k]) for k, v in errs.items() if not v <= 1.5 * own[k]}
    assert not bad, bad


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_freeze_stages_3_runs_the_frozen_lead_without_grad_and_changes_no_trainable_gradient(steps, precision):
    maps5, g5 = steps[(precision, 5)]
    maps3, g3 = steps[(precision, 3)]
    assert all(t.requires_grad for t in maps5)
    assert not maps3[0].requires_grad and maps3[0].grad_fn is None, "the map entering layer2 carries a graph"
    assert all(t.requires_grad for t in maps3[1:])
    assert all(torch.equal(a, b) for a, b in zip(maps5, maps3))
    for k, g in g3.items():
        if k.startswith(("conv1.", "layer1.")):
            assert g is None and g5[k] is not None, k
        else:
            assert g is not None and torch.equal(g, g5[k]), k


def test_training_mode_step_launches_what_it_did(monkeypatch):
    """a training-mode ResNet50 step calls none of the fixed-statistics entry points, and the BatchNorm backward calls
    it makes are one per layer, 53, as before: the new path adds no launch to the existing ones"""
    from ssl4gie_amd import ops
    from ssl4gie_amd.Models.resnet import ResNet50
    calls = {}

    def counted(name):
        fn = getattr(ops, name)

        def wrapper(*a, **k):
            calls[name] = calls.get(name, 0) + 1
            return fn(*a, **k)
        monkeypatch.setattr(ops, name, wrapper)
    for name in ("bn_bwd_frozen", "bn_bwd", "bn_bwd_bits", "bn_bwd_xmask", "bn_coef_stats", "bn_apply_bits"):
        counted(name)
    torch.manual_seed(5)
    m = ResNet50().to(DEV)
    m.set_precision("bf16")
    m.train()
    out = m.forward_maps(torch.randn(4, 3, 64, 64, generator=G(6)).to(DEV))
    out.float().square().mean().backward()
    assert "bn_bwd_frozen" not in calls and "bn_coef_stats" not in calls and "bn_apply_bits" not in calls, calls
    assert sum(calls.values()) == 53 and calls["bn_bwd_xmask"] == 33, calls     # bn1 / bn2 of 16 blocks and the stem
