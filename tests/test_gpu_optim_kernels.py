"""`adamw_arena_kernel` and the three LARS kernels of optim_ops.hip against a plain fp64 reference, per element
(tests/optim_checks.py: the references, the bounds, how their constants were derived and the case list;
tests/test_optim_checks_cpu.py: proof that the checks bite).

The kernels are called through the C ABI (`_lib.load()`) with every buffer in the middle of one that carries 256
guard elements on either side; then one step through each optimizer class — ArenaAdamW (host-counted, with clip_grad,
and with step_count set to 1000), ArenaLARS and RangedLARS — on the toy of tests/test_gpu_optim.py (frozen and
gradient-less parameters, two groups, a conv weight), with the reference started from the flat buffers as they are
before that step and the tables taken from the model and the groups, not from the optimizer.  Same checks, same k.

Run time on an MI355X: 52 tests in 5 s, none above 0.4 s but the last (k_ref of the fp32 evaluation on the GPU, 1.7 s)."""
import pytest
import torch

import optim_checks as oc

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32 = torch.float32
WORST = {}      # worst error / (2^-24 mag) per check over the module (printed by the last test)


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from ssl4gie_amd import _lib
    _lib.load()


def done(rep):
    for n, v in rep.worst.items():
        WORST[n] = max(WORST.get(n, 0.0), v)
    rep.assert_ok()


RUN = {"adamw": oc.run_adamw, "lars": oc.run_lars}
SPECS = {kind: oc.gpu_specs(kind) for kind in oc.KINDS}


def run_group(kind, group):
    rep = oc.Report()
    for grp, a in SPECS[kind]:
        if grp != group:
            continue
        c = oc.make(kind, a)
        o, guard = RUN[kind](c, DEV)
        rep.merge(guard).merge(oc.run_check(c, o))
    done(rep)


@pytest.mark.parametrize("group", oc.groups(SPECS["adamw"]))
def test_adamw_arena(group):
    """both beta pairs, t = 1 .. 100000, both eps, host- and device-counted, ctl[1] = 1 and 0.37, six input families on
    four layouts; `ranges`: each segment alone, [64, end) and [1152, 1280) on small"""
    run_group("adamw", group)


@pytest.mark.parametrize("group", oc.groups(SPECS["lars"]))
def test_lars_arena(group):
    """three (wd, momentum) pairs, a zero and a non-zero momentum buffer, five layouts (300 segments: the second
    workgroup of lars_trust_kernel; 33344 elements: the second trip of the norm loop), all-zero p and all-zero
    g + wd p; `sub`: a sub-range of the arena with seg_start rebased to it"""
    run_group("lars", group)


# ------------------------------------------------------------------ through the optimizer classes
def _model_tables(m, a, groups, default_lr, own=None):
    """start, lr, wd, mat per arena segment from the model and the parameter groups: a parameter is skipped when it
    is in no group (or not one of `own`), frozen, or without a gradient"""
    hyper = {id(p): (g.get("lr", default_lr), g["weight_decay"]) for g in groups for p in g["params"]}
    lr, wd, mat = [], [], []
    for p in a.params:
        on = id(p) in hyper and p.requires_grad and p.grad is not None and (own is None or any(p is q for q in own))
        lr.append(hyper[id(p)][0] if on else -1.0)
        wd.append(hyper[id(p)][1] if on else 0.0)
        mat.append(1.0 if on and p.ndim > 1 else 0.0)
    start = list(a.offsets) + [a.numel]
    pad = [(o + p.numel(), e) for p, o, e in zip(a.params, start[:-1], start[1:]) if o + p.numel() < e]
    return {"start": start, "lr": torch.tensor(lr), "wd": torch.tensor(wd), "mat": torch.tensor(mat), "pad": pad}


def _grads_into_the_arena(m, a, seed):
    """the toy's fake gradients as views of the gradient arena; NaN over the slices of parameters without one"""
    from test_gpu_optim import _fake_grads
    _fake_grads(m, seed)
    ends = list(a.offsets[1:]) + [a.numel]
    for p, o, e in zip(a.params, a.offsets, ends):
        if p.grad is None:
            a.grad[o:e] = float("nan")
        else:
            v = a.grad_view(p)
            v.copy_(p.grad)
            p.grad = v


def _two_groups(m):
    decay = [p for n, p in m.named_parameters() if p.requires_grad and p.ndim > 1]
    no_decay = [p for n, p in m.named_parameters() if p.requires_grad and p.ndim <= 1]
    return [{"params": no_decay, "weight_decay": 0.0, "lr": 3e-3}, {"params": decay, "weight_decay": 0.05}]


def _flat(t, n):
    return torch.zeros(n) if t is None else t.detach().cpu().clone()


@pytest.mark.parametrize("clip", [None, 0.5], ids=["host_counted", "clip_grad"])
def test_arena_adamw_class_steps(clip):
    """step 1 from a fresh optimizer, then step_count = 1000 and step 1001 (with clip_grad: device-counted, the
    coefficient read back from the control block the norm pass wrote)"""
    from test_gpu_optim import _toy
    from ssl4gie_amd.optim import ArenaAdamW
    m = _toy()
    a = m.arena()
    groups = _two_groups(m)
    betas, eps = (0.9, 0.999), 1e-8
    opt = ArenaAdamW(m, [dict(g) for g in groups], lr=2e-2, betas=betas, eps=eps)
    rep = oc.Report()
    for i, t in enumerate((1, 1001)):
        if t == 1001:
            opt.step_count = 1000
        _grads_into_the_arena(m, a, 70 + i)
        tab = _model_tables(m, a, groups, 2e-2)
        n = a.numel
        before = {"p": _flat(a.data, n), "g": _flat(a.grad, n), "m": _flat(opt.exp_avg, n), "v": _flat(opt.exp_avg_sq, n),
                  "lp": a.lp_flat_for_update().detach().cpu().clone()}
        if clip is None:
            opt.step()
        else:
            opt.step(clip_grad=clip)
        torch.cuda.synchronize()
        coef = 1.0 if clip is None else float(opt._gn.ctl[1])
        assert clip is None or 0 < coef < 0.05      # gradients of norm ~ 80 against max_norm 0.5
        assert opt.step_count == t
        c = dict(tab, kind="adamw", layout="toy", family="class", b1=betas[0], b2=betas[1], eps=eps, t=t,
                 mode="host" if clip is None else "dev", coef=coef, lo=0, hi=n, **before)
        o = {"p": _flat(a.data, n), "g": _flat(a.grad, n), "m": _flat(opt.exp_avg, n), "v": _flat(opt.exp_avg_sq, n),
             "lp": a._lp.detach().cpu().clone()}        # the shadow as the kernel left it, before any refresh
        rep.merge(oc.run_check(c, o))
        assert bool(oc.adamw_ref(c)["act"].any()) and not bool(oc.adamw_ref(c)["act"].all())
    done(rep)


@pytest.mark.parametrize("ranged", [False, True], ids=["ArenaLARS", "RangedLARS"])
def test_lars_class_steps(ranged):
    """two steps (a zero, then a non-zero momentum buffer); RangedLARS over the hull of b's weight and bias: its
    momentum buffer is hull-sized and everything outside the hull stays as it is"""
    from test_gpu_optim import _toy
    from ssl4gie_amd.optim import ArenaLARS, RangedLARS
    m = _toy()
    a = m.arena()
    n = a.numel
    if ranged:
        own = [m.b.weight, m.b.bias]
        groups = [{"params": own, "weight_decay": 1e-2}]
        opt = RangedLARS(m, [dict(g) for g in groups], lr=0.1, weight_decay=0.0, momentum=0.9, trust_coefficient=1e-3)
        lo, hi = a.span(own)
    else:
        own = None
        groups = [dict(g, weight_decay=g["weight_decay"] * 0.2) for g in _two_groups(m)]
        opt = ArenaLARS(m, [dict(g) for g in groups], lr=0.3, momentum=0.9, trust_coefficient=1e-3)
        lo, hi = 0, n

    def mu_full():
        full = torch.zeros(n)
        if opt.mu is not None:
            full[lo:hi] = opt.mu.detach().cpu()
        return full
    rep = oc.Report()
    for i in range(2):
        _grads_into_the_arena(m, a, 80 + i)
        tab = _model_tables(m, a, groups, 0.1 if ranged else 0.3, own)
        idx = [j for j, l in enumerate(tab["lr"].tolist()) if l >= 0]
        i0, i1 = (min(idx), max(idx) + 1) if ranged else (0, len(a.params))
        assert (tab["start"][i0], tab["start"][i1]) == (lo, hi)
        before = {"p": _flat(a.data, n), "g": _flat(a.grad, n), "mu": mu_full()}
        opt.step()
        torch.cuda.synchronize()
        c = dict(tab, kind="lars", layout="toy", family="class", momentum=0.9, trust=1e-3, i0=i0, i1=i1, lo=lo, hi=hi,
                 **before)
        rep.merge(oc.run_check(c, {"p": _flat(a.data, n), "g": _flat(a.grad, n), "mu": mu_full()}))
        assert opt.mu.numel() == hi - lo
    done(rep)


def test_zz_k_ref_and_worst_ratios():
    """not a check of the kernels: k_ref of the fp32 torch evaluation on this GPU and the kernels' worst
    error / (2^-24 mag) per check over this module, for optim_checks' table.  The committed K_REF_GPU must be what
    this GPU gives (empty: not yet measured)."""
    k_ref = oc.measure_k_ref(DEV, log=lambda s: None)
    print("\nk_ref (torch on this GPU):", {n: float("%.4g" % v) for n, v in sorted(k_ref.items())})
    print("kernels' worst error / (2^-24 mag):", {n: float("%.3g" % v) for n, v in sorted(WORST.items()) if n in oc.CHECKS})
    for n, v in oc.K_REF_GPU.items():
        assert abs(k_ref[n] - v) <= 0.05 * v, (n, k_ref[n], v)
