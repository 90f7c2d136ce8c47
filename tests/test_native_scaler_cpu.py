"""No GPU needed: the drop-in scaler module's interface (`Models/mae/util/misc.py:251-292` of the reference) and the
host-only parts of the arena norm path."""
import inspect

import pytest
import torch


def test_call_signature_is_the_reference_s():
    from ssl4gie_amd.Models.mae.util import misc
    sig = inspect.signature(misc.NativeScalerWithGradNormCount.__call__)
    got = [(n, p.default) for n, p in sig.parameters.items() if n != "self"]
    assert got == [("loss", inspect.Parameter.empty), ("optimizer", inspect.Parameter.empty), ("clip_grad", None),
                   ("parameters", None), ("create_graph", False), ("update_grad", True)]
    assert all(p.kind is inspect.Parameter.POSITIONAL_OR_KEYWORD for p in sig.parameters.values())
    sig = inspect.signature(misc.get_grad_norm_)
    assert [(n, p.default) for n, p in sig.parameters.items()] == [("parameters", inspect.Parameter.empty),
                                                                   ("norm_type", 2.0)]


def test_state_dict_key_and_round_trip():
    from ssl4gie_amd.Models.mae.util import misc
    assert misc.NativeScalerWithGradNormCount.state_dict_key == "amp_scaler"
    s = misc.NativeScalerWithGradNormCount()
    keys = {"scale", "growth_factor", "backoff_factor", "growth_interval", "_growth_tracker"}  # GradScaler's
    assert set(s.state_dict()) == keys
    saved = {"scale": 1024.0, "growth_factor": 2.0, "backoff_factor": 0.5, "growth_interval": 2000,
             "_growth_tracker": 17}
    s.load_state_dict(saved)
    assert s.state_dict() == saved
    s.load_state_dict({})   # a checkpoint written with AMP disabled
    assert set(s.state_dict()) == keys
    with pytest.raises(KeyError):
        s.load_state_dict({"not_a_scaler_key": 1})


def test_workspace_query_needs_no_gpu():
    from ssl4gie_amd import _lib
    assert _lib.load().ssl4gie_grad_norm_workspace_bytes() > 0


def test_norm_of_a_cpu_model_is_refused():
    from ssl4gie_amd import optim
    from ssl4gie_amd.engine import EngineModule

    class Toy(EngineModule):
        def __init__(self):
            super().__init__()
            self.a = torch.nn.Linear(4, 8)
    m = Toy()
    for p in m.parameters():
        p.grad = torch.ones_like(p)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        optim.get_grad_norm_(m)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        optim.clip_grad_norm_(m, 1.0)


def test_misc_falls_back_to_the_torch_expression_outside_an_arena():
    """parameters that live in no engine arena (here: a plain CPU module): the reference's per-tensor expression"""
    from ssl4gie_amd.Models.mae.util import misc
    lin = torch.nn.Linear(5, 3)
    g = torch.Generator().manual_seed(0)
    for p in lin.parameters():
        p.grad = torch.randn(p.shape, generator=g)
    ref = torch.cat([p.grad.flatten() for p in lin.parameters()]).norm()
    assert torch.allclose(misc.get_grad_norm_(lin.parameters()), ref, rtol=1e-6)
    assert torch.allclose(misc.get_grad_norm_(lin.parameters(), float("inf")),
                          max(p.grad.abs().max() for p in lin.parameters()))
    # the scaler drives a torch optimizer through that path: clip, step, the pre-clip norm comes back
    opt = torch.optim.SGD(lin.parameters(), lr=0.1)
    w0 = lin.weight.detach().clone()
    x = torch.randn(4, 5, generator=g)
    opt.zero_grad()
    scaler = misc.NativeScalerWithGradNormCount()
    assert scaler(lin(x).square().mean(), opt, parameters=lin.parameters(), update_grad=False) is None
    assert torch.equal(lin.weight, w0)
    norm = scaler(lin(x).square().mean(), opt, clip_grad=1e-3, parameters=lin.parameters())
    assert float(norm) > 1e-3
    step = (lin.weight.detach() - w0).norm() / 0.1
    assert float(step) <= 1e-3 * (1 + 1e-5)   # the applied gradient was clipped to norm 1e-3
