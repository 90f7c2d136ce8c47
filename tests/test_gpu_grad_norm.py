"""GPU: the arena gradient-norm / clip / non-finite-skip kernels (`optim.get_grad_norm_`, `optim.clip_grad_norm_`,
`ArenaAdamW.step(clip_grad=, skip_nonfinite=)`) against fp64, torch.nn.utils.clip_grad_norm_ and torch.optim.AdamW.

Two toy EngineModules with fake gradients from a seeded CPU generator (the style of test_gpu_optim.py):

  toy A  ten parameters of 7 ... 2880 elements (several share one 1024-element block of the kernels), a frozen and
         a never-used parameter between active ones, one gradient scaled by 1e-4 and one by 1e3;
  toy B  toy A + Linear(1500, 1400) (2.1 M elements: every block of the fixed-grid norm pass takes more than one
         trip, the last block's range is ragged) + a final 1-element parameter (the last segment of the arena).

Tolerances.  EPS = 2^-24 is half an ulp of fp32.  The norm's bar is max(4 x the error of the reference's own fp32
expression on the same tensors, 8 EPS): the kernel may not be worse than a small multiple of what it replaces, and
8 EPS allows for a different summation tree where the reference happens to land within an ulp.  A clipped gradient
element is (max_norm / (norm + 1e-6)) * g: the norm's bar, plus one add, one division and one multiply on either
side (4 EPS).  The fused AdamW is held to test_gpu_optim.py's own 1e-5 with nothing added."""
import copy

import pytest
import torch

from conftest import rel_err

pytestmark = pytest.mark.gpu
DEV = "cuda"
EPS = 2.0 ** -24
SCALED = {"b.weight": 1e-4, "conv.weight": 1e3}


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from ssl4gie_amd import _lib
    _lib.load()


def _toy(kind):
    from ssl4gie_amd.engine import EngineModule

    class Toy(EngineModule):
        def __init__(self):
            super().__init__()
            self.a = torch.nn.Linear(40, 72)
            self.b = torch.nn.Linear(72, 24)
            self.norm = torch.nn.LayerNorm(24)
            self.frozen = torch.nn.Parameter(torch.randn(3, 5), requires_grad=False)
            self.unused = torch.nn.Parameter(torch.randn(7))  # never receives a gradient
            self.conv = torch.nn.Conv2d(8, 16, 3)
            if kind == "B":
                self.big = torch.nn.Linear(1500, 1400)
                self.last = torch.nn.Parameter(torch.randn(1))
    torch.manual_seed(0)
    return Toy().to(DEV)


def _fake_grads(m, seed):
    g = torch.Generator("cpu").manual_seed(seed)
    for name, p in m.named_parameters():
        if p.requires_grad and name != "unused":
            p.grad = (torch.randn(p.shape, generator=g) * SCALED.get(name, 1.0)).to(DEV)
        else:
            p.grad = None


def _copy_grads(m, ref):
    for p1, p2 in zip(m.parameters(), ref.parameters()):
        p2.grad = None if p1.grad is None else p1.grad.detach().clone()


def _groups(m):
    decay = [p for n, p in m.named_parameters() if p.requires_grad and p.ndim > 1]
    no_decay = [p for n, p in m.named_parameters() if p.requires_grad and p.ndim <= 1]
    return [{"params": no_decay, "weight_decay": 0.0}, {"params": decay, "weight_decay": 0.05}]


def _reference_fp32_norm(params):   # Models/mae/util/misc.py:280-292 restated
    return torch.norm(torch.stack([torch.norm(p.grad.detach(), 2.0) for p in params if p.grad is not None]), 2.0)


_BARS = {}


def _bar(kind):
    """(fp64 norm, error of the reference's fp32 expression, the bar) for the seed-7 gradients of a toy; once"""
    if kind not in _BARS:
        m = _toy(kind)
        _fake_grads(m, 7)
        ref64 = torch.cat([p.grad.double().flatten() for p in m.parameters() if p.grad is not None]).norm().item()
        err_torch = abs(float(_reference_fp32_norm(m.parameters())) - ref64) / ref64
        _BARS[kind] = (ref64, err_torch, max(4.0 * err_torch, 8.0 * EPS))
    return _BARS[kind]


@pytest.mark.parametrize("kind", ["A", "B"])
@pytest.mark.parametrize("through", ["model", "optimizer"])
def test_norm_against_fp64(kind, through):
    from ssl4gie_amd.optim import ArenaAdamW, get_grad_norm_
    ref64, err_torch, bar = _bar(kind)
    m = _toy(kind)
    _fake_grads(m, 7)
    target = m if through == "model" else ArenaAdamW(m, _groups(m), lr=1e-2)
    norm = get_grad_norm_(target)
    assert norm.ndim == 0 and norm.is_cuda and norm.dtype == torch.float32
    err = abs(float(norm) - ref64) / ref64
    print(f"toy {kind} via {through}: kernel rel err {err:.3e}, reference fp32 expression {err_torch:.3e}, bar {bar:.3e}")
    assert err <= bar, f"kernel rel err {err:.3e} vs fp64; the reference's fp32 expression: {err_torch:.3e}; bar {bar:.3e}"


@pytest.mark.parametrize("kind", ["A", "B"])
@pytest.mark.parametrize("through", ["model", "optimizer"])
def test_masked_segments_are_not_read_and_the_norm_is_deterministic(kind, through):
    from ssl4gie_amd.optim import ArenaAdamW, get_grad_norm_
    m = _toy(kind)
    _fake_grads(m, 7)
    target = m if through == "model" else ArenaAdamW(m, _groups(m), lr=1e-2)
    clean = get_grad_norm_(target).clone()
    a = m.arena()
    for frozen_fill, unused_fill in ((float("nan"), 1e30), (1e30, float("nan"))):
        a.grad_view(m.frozen).fill_(frozen_fill)
        a.grad_view(m.unused).fill_(unused_fill)
        first = get_grad_norm_(target).clone()
        second = get_grad_norm_(target).clone()
        state = target._grad_norm(a) if through == "optimizer" else a._grad_norm_state["gn"]
        assert float(state.found_inf) == 0.0
        assert first.view(torch.int32).item() == clean.view(torch.int32).item(), (float(first), float(clean))
        assert second.view(torch.int32).item() == first.view(torch.int32).item()


def test_found_inf_is_decided_per_element():
    """one inf / NaN / -inf in an active gradient sets the flag: in the LAST (1-element) segment of the arena, in
    the middle of the 2.1 M-element one (second trip of a block), and at the end of a small one"""
    from ssl4gie_amd.optim import get_grad_norm_
    m = _toy("B")
    for name, idx, val in (("last", 0, float("inf")), ("big.weight", 1234567, float("nan")),
                           ("a.bias", 71, float("-inf"))):
        _fake_grads(m, 7)
        get_grad_norm_(m)
        gn = m.arena()._grad_norm_state["gn"]
        assert float(gn.found_inf) == 0.0
        dict(m.named_parameters())[name].grad.view(-1)[idx] = val
        get_grad_norm_(m)
        assert float(gn.found_inf) == 1.0, name


@pytest.mark.parametrize("kind", ["A", "B"])
def test_clip_in_place_matches_torch(kind):
    from ssl4gie_amd.optim import clip_grad_norm_, get_grad_norm_
    _, err_torch, bar = _bar(kind)
    m = _toy(kind)
    ref = copy.deepcopy(m)
    _fake_grads(m, 7)
    _copy_grads(m, ref)
    norm0 = float(get_grad_norm_(m))
    before = [None if p.grad is None else p.grad.clone() for p in m.parameters()]
    # not clipping: coefficient exactly 1, nothing written
    ret = clip_grad_norm_(m, 10.0 * norm0)
    assert float(ret) == norm0
    for p, g0 in zip(m.parameters(), before):
        assert (p.grad is None) == (g0 is None)
        assert g0 is None or torch.equal(p.grad, g0)
    # clipping
    ret = float(clip_grad_norm_(m, 0.1 * norm0))
    assert ret == norm0, "the returned norm is the one BEFORE clipping"
    torch.nn.utils.clip_grad_norm_([p for p in ref.parameters()], 0.1 * norm0)
    tol = bar + 4.0 * EPS
    worst = 0.0
    for (n1, p1), p2 in zip(m.named_parameters(), ref.parameters()):
        assert (p1.grad is None) == (p2.grad is None), n1
        if p1.grad is None:
            continue
        d = ((p1.grad.double() - p2.grad.double()).abs() / p2.grad.double().abs().clamp_min(1e-300)).max().item()
        worst = max(worst, d)
        assert d <= tol, f"{n1}: element-wise rel err {d:.3e} > {tol:.3e} (norm bar {bar:.3e}, fp32 expr {err_torch:.3e})"
    print(f"toy {kind}: worst element-wise rel err of a clipped gradient {worst:.3e}, tolerance {tol:.3e}")
    after = float(get_grad_norm_(m))
    assert abs(after - 0.1 * norm0) <= 1e-5 * 0.1 * norm0


@pytest.mark.parametrize("kind", ["A", "B"])
def test_fused_adamw_with_clip_matches_torch(kind):
    from ssl4gie_amd.optim import ArenaAdamW
    m = _toy(kind)
    ref = copy.deepcopy(m)
    m.arena()
    opt = ArenaAdamW(m, _groups(m), lr=1e-2, betas=(0.9, 0.95))
    topt = torch.optim.AdamW(_groups(ref), lr=1e-2, betas=(0.9, 0.95))
    frozen0, unused0 = m.frozen.detach().clone(), m.unused.detach().clone()
    clip = 1000.0   # the norms are about 3.4e4 (the 1e3-scaled convolution gradient): clipping is live
    for step in range(4):
        _fake_grads(m, 10 + step)
        _copy_grads(m, ref)
        if step == 2:  # a learning-rate schedule edits param_groups in place
            for g in opt.param_groups + topt.param_groups:
                g["lr"] = 5e-3
        before = [None if p.grad is None else p.grad.clone() for p in m.parameters()]
        opt.step(clip_grad=clip)
        assert float(opt.last_grad_norm) > 10 * clip and float(opt.last_found_inf) == 0.0
        for (n, p), g0 in zip(m.named_parameters(), before):   # the fused path leaves p.grad unscaled
            assert g0 is None or torch.equal(p.grad, g0), n
        tn = torch.nn.utils.clip_grad_norm_([p for p in ref.parameters()], clip)
        assert abs(float(opt.last_grad_norm) - float(tn)) <= 1e-5 * float(tn)
        topt.step()
    for (n1, p1), (n2, p2) in zip(m.named_parameters(), ref.named_parameters()):
        assert rel_err(p1, p2) < 1e-5, n1
    assert torch.equal(m.frozen, frozen0) and torch.equal(m.unused, unused0)
    assert opt.state_dict()["step_count"] == 4


def test_nonfinite_step_is_skipped_entirely():
    from ssl4gie_amd.optim import ArenaAdamW
    m = _toy("A")
    ref = copy.deepcopy(m)
    a = m.arena()
    opt = ArenaAdamW(m, _groups(m), lr=1e-2, betas=(0.9, 0.95))
    topt = torch.optim.AdamW(_groups(ref), lr=1e-2, betas=(0.9, 0.95))
    # step 1: finite
    _fake_grads(m, 30)
    _copy_grads(m, ref)
    opt.step(skip_nonfinite=True)
    topt.step()
    assert float(opt.last_found_inf) == 0.0
    torch.cuda.synchronize()
    snap = (a.data.clone(), opt.exp_avg.clone(), opt.exp_avg_sq.clone(), a._lp.clone())
    # step 2: one inf in an active gradient -> nothing moves, the bias-correction step does not advance
    _fake_grads(m, 31)
    m.b.weight.grad[3, 5] = float("inf")
    opt.step(skip_nonfinite=True)
    assert float(opt.last_found_inf) == 1.0
    now = (a.data, opt.exp_avg, opt.exp_avg_sq, a._lp)
    for name, x, y in zip(("arena", "exp_avg", "exp_avg_sq", "bf16 shadow"), snap, now):
        assert torch.equal(x, y), name
    # step 3: finite; torch's AdamW never saw step 2
    _fake_grads(m, 32)
    _copy_grads(m, ref)
    opt.step(skip_nonfinite=True)
    topt.step()
    assert float(opt.last_found_inf) == 0.0
    for (n1, p1), (n2, p2) in zip(m.named_parameters(), ref.named_parameters()):
        assert rel_err(p1, p2) < 1e-5, n1
    assert opt.state_dict()["step_count"] == 2
    w = m.a.weight
    o = a._index[id(w)]
    assert torch.equal(a._lp[o:o + w.numel()], w.detach().flatten().to(torch.bfloat16))
    # a plain step() afterwards keeps using the device-side count
    _fake_grads(m, 33)
    _copy_grads(m, ref)
    opt.step()
    topt.step()
    for (n1, p1), (n2, p2) in zip(m.named_parameters(), ref.named_parameters()):
        assert rel_err(p1, p2) < 1e-5, n1
    assert opt.step_count == 3


def test_no_host_synchronisation():
    """steady state: the segment tables and the bf16 shadow are built once, at the first step with a given set of
    gradients (engine.ParamArena._refresh_lp creates its tables with blocking copies), so one warm-up update runs
    outside the checked region; the checked calls get NEW gradient tensors, adopted into the arena inside it"""
    from ssl4gie_amd.optim import ArenaAdamW, clip_grad_norm_
    torch.cuda.set_sync_debug_mode("error")
    try:
        try:
            torch.ones(1, device=DEV).item()
            honoured = False
        except RuntimeError:
            honoured = True
    finally:
        torch.cuda.set_sync_debug_mode("default")
    if not honoured:
        pytest.skip("torch.cuda.set_sync_debug_mode('error') does not flag a .item() in this torch build on ROCm: "
                    "there is nothing to observe a synchronisation with")
    m = _toy("B")
    m.arena()
    opt = ArenaAdamW(m, _groups(m), lr=1e-2, betas=(0.9, 0.95))
    _fake_grads(m, 50)
    clip_grad_norm_(m, 1000.0)
    opt.step(clip_grad=1000.0, skip_nonfinite=True)
    _fake_grads(m, 51)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        norm = clip_grad_norm_(m, 1000.0)
        opt.step(clip_grad=1000.0, skip_nonfinite=True)
        found = opt.last_found_inf
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert float(norm) > 0 and float(found) == 0.0


def test_overlap_backward_refuses_the_options():
    from ssl4gie_amd.optim import ArenaAdamW
    m = _toy("A")
    _fake_grads(m, 7)
    opt = ArenaAdamW(m, _groups(m), lr=1e-2, overlap_backward=True)
    with pytest.raises(ValueError):
        opt.step(clip_grad=1.0)
    with pytest.raises(ValueError):
        opt.step(skip_nonfinite=True)


# ---------------------------------------------------------------------------------------------------------------
# through bare parameters: `Models/mae/util/misc.py` is handed `model.parameters()`, finds their arena
# (engine.arena_of) and builds its own segment mask; with an optimizer that is not ArenaAdamW the scaler runs the
# norm kernel, the scale kernel when clipping, then optimizer.step()
# ---------------------------------------------------------------------------------------------------------------
def _arena_block(m):
    """the control block of the norms taken over the model's arena (not through an optimizer)"""
    st = m.arena()._grad_norm_state
    return None if st is None else st["gn"].ctl


def _is_view_of(t, block):
    return block is not None and t.is_cuda and t.data_ptr() == block.data_ptr()


@pytest.mark.parametrize("kind", ["A", "B"])
def test_misc_get_grad_norm_over_model_parameters(kind):
    from ssl4gie_amd.Models.mae.util import misc
    from ssl4gie_amd.optim import get_grad_norm_
    ref64, err_torch, bar = _bar(kind)
    m = _toy(kind)
    m.arena()
    _fake_grads(m, 7)
    norm = misc.get_grad_norm_(m.parameters())
    assert norm.ndim == 0 and norm.dtype == torch.float32
    assert _is_view_of(norm, _arena_block(m)), "the arena kernel ran, not the per-tensor torch expression"
    err = abs(float(norm) - ref64) / ref64
    print(f"toy {kind} via misc: kernel rel err {err:.3e}, reference fp32 expression {err_torch:.3e}, bar {bar:.3e}")
    assert err <= bar, f"kernel rel err {err:.3e} vs fp64; the reference's fp32 expression: {err_torch:.3e}; bar {bar:.3e}"
    bits = norm.view(torch.int32).item()
    assert get_grad_norm_(m).view(torch.int32).item() == bits   # same tables, same kernel, same bits

    # a strict subset: a matrix that shares a block with its neighbours, the 1e-4-scaled one, a 24-element vector
    # (toy B: and the last, 1-element segment); everything else, the dominant 1e3-scaled gradient included, is
    # masked out
    subset = [m.a.weight, m.b.weight, m.norm.bias] + ([m.last] if kind == "B" else [])
    sub64 = torch.cat([p.grad.double().flatten() for p in subset]).norm().item()
    sub_torch = abs(float(_reference_fp32_norm(subset)) - sub64) / sub64
    sub_bar = max(4.0 * sub_torch, 8.0 * EPS)
    got = float(misc.get_grad_norm_(subset))
    err = abs(got - sub64) / sub64
    print(f"toy {kind} subset: kernel rel err {err:.3e}, reference fp32 expression {sub_torch:.3e}, bar {sub_bar:.3e}")
    assert err <= sub_bar, f"subset: kernel rel err {err:.3e}; fp32 expression {sub_torch:.3e}; bar {sub_bar:.3e}"
    assert abs(got - ref64) / ref64 > 1e-3, "the subset's norm is not the whole model's"
    one = float(misc.get_grad_norm_(m.b.bias))       # a single tensor, as the reference accepts
    assert abs(one - m.b.bias.grad.double().norm().item()) <= 8.0 * EPS * one
    # and back: the mask is rebuilt, the whole model's norm returns to the bit
    assert misc.get_grad_norm_(m.parameters()).view(torch.int32).item() == bits


@pytest.mark.parametrize("kind", ["A", "B"])
def test_native_scaler_drives_a_torch_optimizer_over_the_arena(kind):
    """torch.optim.AdamW on parameters that live in an engine arena, driven by the scaler with
    `parameters=model.parameters()`: against clip_grad_norm_ + torch AdamW on a copy outside any arena"""
    from ssl4gie_amd.Models.mae.util import misc
    ref64, err_torch, bar = _bar(kind)
    m = _toy(kind)
    ref = copy.deepcopy(m)
    m.arena()
    opt = torch.optim.AdamW(_groups(m), lr=1e-2, betas=(0.9, 0.95))
    topt = torch.optim.AdamW(_groups(ref), lr=1e-2, betas=(0.9, 0.95))
    scaler = misc.NativeScalerWithGradNormCount()
    clip = 1000.0   # the norms are about 3.4e4: clipping is live
    tol = bar + 4.0 * EPS

    def loss():     # a leaf: its backward touches no parameter, the fake gradients stay
        return torch.zeros((), device=DEV, requires_grad=True)

    for step, seed in enumerate((7, 11, 12)):
        _fake_grads(m, seed)
        _copy_grads(m, ref)
        assert scaler(loss(), opt, clip_grad=clip, parameters=m.parameters(), update_grad=False) is None
        norm = scaler(loss(), opt, clip_grad=clip, parameters=m.parameters())
        assert _is_view_of(norm, _arena_block(m)), "the arena kernels ran, not torch's clip_grad_norm_"
        torch.nn.utils.clip_grad_norm_([p for p in ref.parameters()], clip)
        topt.step()
        assert float(norm) > 10 * clip
        if step == 0:   # the seed-7 gradients, whose bar is known: p.grad is clipped in place, as torch leaves it
            err = abs(float(norm) - ref64) / ref64
            assert err <= bar, f"pre-clip norm: rel err {err:.3e} vs fp64; fp32 expression {err_torch:.3e}; bar {bar:.3e}"
            worst = 0.0
            for (n1, p1), p2 in zip(m.named_parameters(), ref.parameters()):
                assert (p1.grad is None) == (p2.grad is None), n1
                if p1.grad is not None:
                    d = ((p1.grad.double() - p2.grad.double()).abs()
                         / p2.grad.double().abs().clamp_min(1e-300)).max().item()
                    worst = max(worst, d)
            print(f"toy {kind}: worst element-wise rel err of a clipped gradient {worst:.3e}, tolerance {tol:.3e}")
            assert worst <= tol, (worst, tol, err_torch)
    for (n1, p1), (n2, p2) in zip(m.named_parameters(), ref.named_parameters()):
        assert rel_err(p1, p2) < 1e-5, n1
    assert m.arena().intact(), "torch's optimizer updated the arena's views in place"

    # without clip_grad: the norm comes back, p.grad is not touched, the step is taken; `parameters` left out:
    # the optimizer's own
    _fake_grads(m, 13)
    _copy_grads(m, ref)
    norm = scaler(loss(), opt)
    grads = [p.grad for p in ref.parameters() if p.grad is not None]
    r64 = torch.cat([g.double().flatten() for g in grads]).norm().item()
    e32 = abs(float(_reference_fp32_norm(ref.parameters())) - r64) / r64
    assert _is_view_of(norm, _arena_block(m))
    assert abs(float(norm) - r64) / r64 <= max(4.0 * e32, 8.0 * EPS), (float(norm), r64, e32)
    for p1, p2 in zip(m.parameters(), ref.parameters()):
        assert p1.grad is None or torch.equal(p1.grad, p2.grad)
    topt.step()
    for (n1, p1), (n2, p2) in zip(m.named_parameters(), ref.named_parameters()):
        assert rel_err(p1, p2) < 1e-5, n1
